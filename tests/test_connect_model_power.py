"""What the connection case set (tests/connect_cases.py) reaches, on the CPU: every fault switch of tests/connect_model.py is noticed
by a named case (one is inert by construction and shown to be); the verdicts and node counts of the textbook shapes are pinned; no
constructed case ends unknown except the budget and depth cases; the group cases tie what they should; and the golden sample
tests/test_gpu_connect.py enumerates shows all four read verdicts -- the condition that test rests on."""
import numpy as np
import pytest

from tests import connect_cases as CC
from tests import connect_model as M
from tests.tactics_cases import diagram

S0 = 9
INERT = ("no_root_joined",)

# fault switch -> (how the case is run, its name, cut_libs): a run whose model output differs with the switch on
NOTICED = {
    "desc_order": ("asked", "jump_b", 1), "no_attacker_pass": ("asked", "diagonal_b", 1), "pass_only_ko": ("asked", "tiger_corner_b", 1),
    "defender_passes": ("asked", "jump_b", 1), "joined_wrong_anchor": ("asked", "bamboo_b", 1), "y_capture_not_cut": ("region", "ko_b", 1),
    "common_libs_only": ("asked", "knight_b", 1), "no_cutting_chains": ("asked", "cutter_atari_b", 1),
    "cut_libs_off_by_one": ("asked", "crosscut_b", 1), "cutting_not_in_m": ("asked", "cutter_atari_b", 1),
    "no_second_order": ("asked", "diagonal_b", 1), "no_inner_chains": ("enumerated", "false_join_b", 1),
    "anchors_unordered": ("asked", "diagonal_rev_b", 1), "colours_mixed": ("asked", "two_colour_ask_b", 1),
    "shared_counter": ("asked", "peep_b", 1), "d_always": ("asked", "jump_edge_b", 1), "outside_region": ("asked", "jump_b", 1),
    "rules_ignored": ("asked", "fill_b", 1), "no_root_ko": ("region", "ko_w", 1), "ko_wrong_side": ("region", "ko_w", 1),
    "padding_read": ("enumerated", "diagonal_b", 1), "groups_tie_unsettled": ("enumerated", "jump_b", 1),
    "groups_not_transitive": ("enumerated", "chain3_b", 1), "groups_across_colours": ("asked", "peep_b", 1),
}


def _one(mode, name, fault=None, rules=1, cut_libs=1, S=S0):
    """the model's outputs of one named case"""
    names, recs, ask, region, has = CC.case_records(S)
    k = names.index(name)
    kw = dict(rules=rules, cut_libs=cut_libs, max_region=CC.MAX_REGION, max_nodes=CC.MAX_NODES, fault=fault)
    if mode == "asked":
        kw["ask"] = ask[k:k + 1]
    elif mode == "region":
        kw["ask"], kw["region"] = ask[k:k + 1], region[k:k + 1]
    m = M.connect(S, recs[k:k + 1], **kw)
    return int(m["n_pairs"][0]), m["rows"][0].tolist(), m["regions"][0].tolist(), m["groups"][0].tolist(), m["counts"][0].tolist()


def test_every_fault_switch_has_a_case():
    assert sorted(list(NOTICED) + list(INERT)) == sorted(M.FAULTS) and not set(NOTICED) & set(INERT)


@pytest.mark.parametrize("fault", sorted(NOTICED))
def test_fault_is_noticed(fault):
    mode, name, cut_libs = NOTICED[fault]
    assert _one(mode, name, cut_libs=cut_libs) != _one(mode, name, fault, cut_libs=cut_libs), (fault, mode, name)


@pytest.mark.parametrize("S", (5, 9))
def test_the_root_joined_switch_is_inert(S):
    """no_root_joined (tests/connect_model.py argues why): a pair is two different chains at the root of either query"""
    for rules in (1, 0):
        for base, bad in ((CC.asked_model(S, rules), CC.asked_model(S, rules, "no_root_joined")),
                          (CC.enumerated_model(S, rules), CC.enumerated_model(S, rules, "no_root_joined"))):
            assert all(np.array_equal(a, b) for a, b in zip(base["rows"], bad["rows"]))
            assert all(np.array_equal(a, b) for a, b in zip(base["groups"], bad["groups"]))


@pytest.mark.parametrize("S", (7, 9))
@pytest.mark.parametrize("name", sorted(CC.TABLE))
def test_textbook_shapes(name, S):
    """the issue's table at 7x7 and 9x9: rules = 1, cut_libs 1, the default region, black to move and white to move"""
    rows, (p, q), word, nodes_a, nodes_d = CC.TABLE[name]
    b, w = diagram(S, rows)
    pq = (p[1] * S + p[0], q[1] * S + q[0])
    for wtp in (False, True):
        rec = M.build_record(S, b, w, wtp)
        asked = M.connect(S, rec[None], ask=[pq], rules=1, cut_libs=1)["rows"][0]
        listed = M.connect(S, rec[None], rules=1, cut_libs=1)["rows"][0]
        assert len(asked) == 1 and asked[0, :3].tolist() == [pq[0], pq[1], 1] and M.verdict(asked[0]) == word, (name, asked.tolist())
        if word == "open":
            assert asked[0, 5] == 0 and asked[0, 8:].tolist() == [-1, -1, 0, 0] and asked[0].tolist() not in listed.tolist()
        else:
            assert asked[0, 10:].tolist() == [nodes_a, nodes_d or 0], (name, asked.tolist())
            assert asked[0].tolist() in listed.tolist(), (name, "enumerated")
    P = lambda x, y: y * S + x                                                           # noqa: E731
    if name == "diagonal":
        assert asked[0, 5] == 6
    if name == "jump":
        assert asked[0, 8:10].tolist() == [P(2, 2), P(2, 1)]         # the cut at the point between; the first join found is above it
    if name == "peep":
        assert asked[0, 8] == P(1, 2)


def test_cut_libs_moves_the_cutting_chains():
    """cutter_atari at cut_libs 0 has no link point and reads open; the peep at cut_libs 2 has nine empty points in its region"""
    names, recs, ask, region, has = CC.case_records(S0)
    k = names.index("cutter_atari_b")
    row = M.connect(S0, recs[k:k + 1], ask=ask[k:k + 1], cut_libs=0)["rows"][0][0]
    assert M.verdict(row) == "open" and row[4] == 0 and row[7] == 0
    assert CC.asked_model(S0, 1)["rows"][k][0][7] == 1
    k = names.index("peep_b")
    row = M.connect(S0, recs[k:k + 1], ask=ask[k:k + 1], cut_libs=2, max_region=9, max_nodes=256)["rows"][0][0]
    assert row[5] == 9 and row[7] == 1 and row[6] == M.A_UNKNOWN and row[10] == 257


def test_verdicts_of_the_other_named_cases():
    """the ko: white to play may not retake and black joins, with black to play white's capture cuts; fill: cut under rules = 0,
    connected under rules = 1; the knight's move and the far stones are open; the five ways to ask for no pair"""
    names = CC.case_records(S0)[0]
    asked = {n: CC.asked_model(S0, 1)["rows"][i][0].tolist() for i, n in enumerate(names)}
    asked0 = {n: CC.asked_model(S0, 0)["rows"][i][0].tolist() for i, n in enumerate(names)}
    pick, reg = CC.region_model(S0, 1)
    given = {names[k]: reg["rows"][i][0].tolist() for i, k in enumerate(pick)}
    P = lambda x, y: y * S0 + x                                                          # noqa: E731
    assert M.verdict(given["ko_w"]) == "connected" and given["ko_w"][10:] == [3, 0]
    assert M.verdict(given["ko_b"]) == "unsettled" and given["ko_b"][8:10] == [P(1, 1), P(1, 1)]
    assert M.verdict(asked["fill_b"]) == "connected" and M.verdict(asked0["fill_b"]) == "cut" and asked0["fill_b"][8:10] == [S0 * S0, -1]
    assert asked["diagonal_rev_b"] == asked["diagonal_b"]
    assert M.verdict(asked["knight_b"]) == "open" and asked["knight_b"][3:6] == [0, 4, 10]
    assert M.verdict(asked["stones_far_b"]) == "open" and asked["stones_far_b"][3:] == [0, 0, 0, M.OPEN, 0, -1, -1, 0, 0]
    for n in ("empty_point_b", "point_n_w", "negative_b", "two_colour_ask_w", "one_chain_b"):
        assert asked[n] == M.NO_PAIR_ROW, n


def test_group_cases():
    """chain3 / side3: A-B and B-C connected, A-C not NEAR (two rows), one group of three chains; jump: one unsettled pair, two
    groups; two_colours: a black and a white group in one map; an open row sets flag 2 and ties nothing"""
    names = CC.case_records(S0)[0]
    en, asked = CC.enumerated_model(S0, 1), CC.asked_model(S0, 1)
    P = lambda x, y: y * S0 + x                                                          # noqa: E731
    for name, pts in (("chain3_b", [P(1, 1), P(2, 2), P(3, 3)]), ("side3_w", [P(0, 0), P(2, 0), P(4, 0)])):
        k = names.index(name)
        assert [M.verdict(r) for r in en["rows"][k]] == ["connected", "connected"] and en["rows"][k][:, :2].tolist() == [pts[:2], pts[1:]]
        assert en["counts"][k].tolist() == [3, 1, 2, 0] and [en["groups"][k][a] for a in pts] == [pts[0]] * 3
        assert (np.delete(en["groups"][k], pts) == -1).all()
        assert M.verdict(asked["rows"][k][0]) == "open" and asked["counts"][k].tolist() == [3, 3, 0, M.FLAG_UNDECIDED]
    k = names.index("jump_b")
    assert en["counts"][k].tolist() == [2, 2, 0, 0] and sorted(set(en["groups"][k].tolist())) == [-1, P(1, 2), P(3, 2)]
    k = names.index("two_colours_b")
    assert en["counts"][k].tolist() == [4, 2, 2, 0] and sorted(set(en["groups"][k].tolist())) == [-1, P(0, 0), P(3, 0)]
    cut = CC.enumerated_model(S0, 1, max_pairs=2)
    k = names.index("ko_b")
    assert cut["counts"][k][3] == M.FLAG_CUT_TABLE and cut["counts"][k][1] > en["counts"][k][1]


@pytest.mark.parametrize("S", M.SIZES)
def test_no_constructed_case_ends_unknown(S):
    """asked, enumerated and in the given regions, for both rule sets; the budget and depth cases are run apart"""
    for rules in (1, 0):
        for m in (CC.asked_model(S, rules), CC.enumerated_model(S, rules), CC.region_model(S, rules)[1]):
            for rows in m["rows"]:
                assert not (rows[:, 6] & (M.A_UNKNOWN | M.D_UNKNOWN)).any(), (S, rules, rows.tolist())


def test_budget_and_depth_cases_end_unknown():
    names, recs, ask, region, has = CC.case_records(S0)
    k = names.index("diagonal_b")
    full = CC.asked_model(S0, 1)["rows"][k][0]
    nodes = int(full[10])
    assert nodes == 145
    less = M.connect(S0, recs[k:k + 1], ask=ask[k:k + 1], max_nodes=nodes - 1)["rows"][0][0]
    same = M.connect(S0, recs[k:k + 1], ask=ask[k:k + 1], max_nodes=nodes)["rows"][0][0]
    assert less[6] == M.A_UNKNOWN and less[8:].tolist() == [-1, -1, nodes, 0] and same.tolist() == full.tolist()
    deep = CC.deep_model()
    row = deep["rows"][0][0]
    assert row[6] == M.A_UNKNOWN and row[10] == 82 and deep["depths"][0][0, 0] == M.MAX_DEPTH


def test_golden_sample_shows_every_verdict():
    """what tests/test_gpu_connect.py::test_golden_sample_enumerated rests on: an all-`unknown` reader cannot pass there"""
    seen, pairs, tied = set(), 0, 0
    for S in M.SIZES:
        m = CC.golden_model(S)
        pairs += int(m["n_pairs"].sum())
        tied += sum(int(c[0] - c[1]) for c in m["counts"])
        for rows in m["rows"]:
            for row in rows:
                seen.add(M.verdict(row))
    assert seen == {"connected", "unsettled", "cut", "unknown"} and pairs >= 100 and tied > 0, (seen, pairs, tied)
