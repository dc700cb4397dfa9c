"""What the life-and-death case set (tests/solve_cases.py) reaches, on the CPU: every fault switch of tests/solve_model.py is noticed
by a named case; no constructed case ends unknown except the budget and depth cases; the model agrees with tests/tactics_model.py on
chains in atari and with tests/life_model.py at the roots; and the golden plies tests/test_gpu_solve.py enumerates are decided, at
their budget, for at least half of their rows -- the condition that test rests on."""
import numpy as np
import pytest

from tests import life_model as LM
from tests import solve_cases as SC
from tests import solve_model as M
from tests import tactics_model as TM

S0 = 7                                                               # the smallest size that holds every constructed case

# fault switch -> (how the case is run, its name): a run whose model output differs with the switch on
NOTICED = {
    "desc_order": ("asked", "square_four_b"), "pass_first": ("asked", "straight_three_b"), "no_pass": ("asked", "seki_b"),
    "attacker_passes": ("region", "connect_small_b"), "no_wait": ("asked", "straight_three_b"), "no_inner_chains": ("asked", "seki_b"), "alive_root_only": ("asked", "straight_four_b"),
    "alive_attacker_colour": ("asked", "straight_four_b"), "ko_wrong_side": ("region", "ko_w"), "no_root_ko": ("region", "ko_w"),
    "root_ko_always": ("region", "ko_b"), "depth_off_by_one": ("deep", None), "shared_counter": ("asked", "connect_b"),
    "d_always": ("asked", "two_eyes_b"), "outside_region": ("region", "connect_small_b"), "rules_ignored": ("asked", "connect_b"),
    "flag_as_stone": ("asked", "open_b"), "padding_read": ("enumerated", "two_eyes_w"),
}


def _one(mode, name, fault=None):
    """the model's table of one named case"""
    if mode == "deep":
        m = SC.deep_model(fault)
    else:
        names, recs, ask, region, has = SC.case_records(S0)
        k = names.index(name)
        kw = dict(rules=1, max_region=SC.MAX_REGION, max_nodes=SC.MAX_NODES, fault=fault)
        if mode == "asked":
            kw["ask"] = ask[k:k + 1]
        elif mode == "region":
            kw["ask"], kw["region"] = ask[k:k + 1], region[k:k + 1]
        m = M.solve(S0, recs[k:k + 1], **kw)
    return int(m["n_targets"][0]), m["rows"][0].tolist(), m["regions"][0].tolist()


def test_every_fault_switch_has_a_case():
    assert sorted(NOTICED) == sorted(M.FAULTS)


@pytest.mark.parametrize("fault", M.FAULTS)
def test_fault_is_noticed(fault):
    mode, name = NOTICED[fault]
    assert _one(mode, name) != _one(mode, name, fault), (fault, mode, name)


def test_the_pass_is_what_keeps_the_seki_alive():
    """the seki reads alive, and a reader without the defender's pass kills it"""
    (_, rows, _), (_, faulty, _) = _one("asked", "seki_b"), _one("asked", "seki_b", "no_pass")
    assert SC.verdict(rows[0]) == "alive" and SC.verdict(faulty[0]) != "alive"


def test_rules_and_region_change_the_verdict():
    names = SC.case_records(S0)[0]
    k = names.index("connect_b")
    assert SC.verdict(SC.asked_model(S0, 1)["rows"][k][0]) == "unsettled" and SC.asked_model(S0, 1)["rows"][k][0][4:6].tolist() == [4, 4]
    assert SC.verdict(SC.asked_model(S0, 0)["rows"][k][0]) == "dead"
    pick, m = SC.region_model(S0, 1)
    small = list(pick).index(names.index("connect_small_b"))
    assert SC.verdict(m["rows"][small][0]) == "alive" and m["rows"][small][0][2] == 2
    kb, kw = list(pick).index(names.index("ko_b")), list(pick).index(names.index("ko_w"))
    assert SC.verdict(m["rows"][kb][0]) != "alive" and SC.verdict(m["rows"][kw][0]) == "alive"     # white to play may not retake


def test_verdicts_of_the_other_named_cases():
    """two eyes: alive at the root, nodes 1 (asked through a stone that is not the anchor); straight four: alive as it stands;
    the nakade with an eye each: dead, by a kill that captures and replays inside the eye; open, no stone"""
    names = SC.case_records(S0)[0]
    rows = {n: SC.asked_model(S0, 1)["rows"][i][0].tolist() for i, n in enumerate(names)}
    assert rows["two_eyes_b"] == [1, 1, 2, 0, -1, -1, 1, 0]
    assert SC.verdict(rows["straight_four_b"]) == "alive" and rows["straight_four_b"][6] > 1
    assert SC.verdict(rows["nakade_b"]) == "dead" and rows["nakade_b"][4] == 2
    assert SC.verdict(rows["open_b"]) == "open" and rows["open_b"][4:] == [-1, -1, 0, 0]
    assert rows["no_stone_b"] == rows["outside_w"] == [-1, 0, 0, M.NO_STONE, -1, -1, 0, 0]


def test_verdicts_of_the_killable_eyes():
    """straight three and bulky five: unsettled, with the vital point as both kill_move and live_move; square four: dead.  Each
    kill ends with the defender capturing ONE stone inside its last eye and the attacker's replay on that point, which the one-stone
    ko approximation forbids for a ply: the attacker's wait is what reads them, and without it (`no_wait`) all three read alive.
    Under rules = 0 the inherited rule forbids the attacker's moves into the eye, and they read alive as well: the verdicts hold for
    the chosen rule set."""
    names, recs, ask, _, _ = SC.case_records(S0)
    rows = {n: SC.asked_model(S0, 1)["rows"][i][0].tolist() for i, n in enumerate(names)}
    got = {n: (SC.verdict(rows[n + "_b"]), rows[n + "_b"][4], rows[n + "_b"][5]) for n in ("straight_three", "bulky_five", "square_four")}
    assert got == {"straight_three": ("unsettled", 1, 1), "bulky_five": ("unsettled", 1, 1), "square_four": ("dead", got["square_four"][1], -1)}, got
    assert got["square_four"][1] >= 0
    for n in got:
        k = names.index(n + "_b")
        m = M.solve(S0, recs[k:k + 1], ask=ask[k:k + 1], max_region=SC.MAX_REGION, max_nodes=SC.MAX_NODES, fault="no_wait")
        assert SC.verdict(m["rows"][0][0]) == "alive", n


@pytest.mark.parametrize("S", M.SIZES)
def test_no_constructed_case_ends_unknown(S):
    """asked, enumerated and in the given regions, for both rule sets; the budget and depth cases are run apart"""
    for rules in (1, 0):
        for m in (SC.asked_model(S, rules), SC.enumerated_model(S, rules), SC.region_model(S, rules)[1]):
            for rows in m["rows"]:
                assert not (rows[:, 3] & (M.A_UNKNOWN | M.D_UNKNOWN)).any(), (S, rules, rows.tolist())


def test_budget_and_depth_cases_end_unknown():
    names, recs, ask, region, has = SC.case_records(S0)
    k = names.index("bulky_five_b")
    nodes = int(SC.asked_model(S0, 1)["rows"][k][0][6])
    less = M.solve(S0, recs[k:k + 1], ask=ask[k:k + 1], max_region=SC.MAX_REGION, max_nodes=nodes - 1)["rows"][0][0]
    same = M.solve(S0, recs[k:k + 1], ask=ask[k:k + 1], max_region=SC.MAX_REGION, max_nodes=nodes)["rows"][0][0]
    assert less[3] == M.A_UNKNOWN and less[6] == nodes and same.tolist() == SC.asked_model(S0, 1)["rows"][k][0].tolist()
    deep = SC.deep_model()
    assert deep["rows"][0][0, 3] == M.A_UNKNOWN and deep["rows"][0][0, 6] < SC.DEEP_NODES and deep["depths"][0][0, 0] == M.MAX_DEPTH


@pytest.mark.parametrize("S", (5, 7, 9))
def test_agrees_with_the_tactics_model_on_chains_in_atari(S):
    """a chain with one liberty that the tactics reader's query A captures is DEAD in query A here, under the same rule set
    (rules = 0), wherever its default region is closed (listed by the enumeration); on the golden plies and the case records"""
    seen = 0
    for recs in (SC.golden_sample(S), SC.case_records(S)[1]):
        t = TM.tactics(S, recs)
        v = M.solve(S, recs, rules=0, max_region=SC.GOLDEN_REGION, max_nodes=SC.MAX_NODES, max_targets=M.MAX_TARGETS)
        for i in range(len(recs)):
            mine = {int(r[0]): r for r in v["rows"][i]}
            for c in t["rows"][i]:
                if c[3] == 1 and c[4] & TM.A_CAPTURED and int(c[0]) in mine:
                    seen += 1
                    assert mine[int(c[0])][3] & M.A_DEAD, (S, i, c.tolist(), mine[int(c[0])].tolist())
    assert seen >= 3, seen


@pytest.mark.parametrize("S", M.SIZES)
def test_agrees_with_the_life_model_at_the_roots(S):
    """no enumerated chain is pass-alive, every chain left out is pass-alive or has a default region outside 1..max_region, and an
    asked pass-alive chain is ALIVE after one node"""
    for recs in (SC.golden_sample(S), SC.case_records(S)[1]):
        v = M.solve(S, recs, rules=1, max_region=SC.GOLDEN_REGION, max_nodes=1, max_targets=M.MAX_TARGETS)
        for i, rec in enumerate(recs):
            sets, _, _ = LM.record_life(S, rec)
            alive = set(LM.points_of(sets[0], S * S)) | set(LM.points_of(sets[1], S * S))
            listed = {int(r[0]) for r in v["rows"][i]}
            assert not listed & alive, (S, i)
            _, chains = TM.chain_table(S, rec)
            for a in sorted(alive)[:2]:
                row = M.record_solve(S, rec, a, None, 1, M.MAX_REGION, 1)[0][0]
                assert row[3] in (0, M.OPEN) and (row[3] == M.OPEN or row[6] == 1), (S, i, a, row.tolist())
            for c in chains:                                         # the chains with one or two liberties: small enough to check all
                a = int(c[0])
                if a not in listed and a not in alive:
                    row = M.record_solve(S, rec, a, None, 1, SC.GOLDEN_REGION, 1)[0][0]
                    assert row[3] == M.OPEN, (S, i, a, row.tolist())


@pytest.mark.parametrize("S", M.SIZES)
def test_golden_plies_are_decided_for_at_least_half_of_their_rows(S):
    """what tests/test_gpu_solve.py::test_golden_plies_enumerated rests on: "unknown everywhere" cannot pass there"""
    m = SC.golden_model(S)
    rows = np.concatenate(m["rows"])
    unknown = int(((rows[:, 3] & (M.A_UNKNOWN | M.D_UNKNOWN)) != 0).sum())
    assert len(SC.golden_sample(S)) <= 64 and len(rows) >= 10 and 2 * unknown <= len(rows), (S, len(rows), unknown)
    assert (m["n_targets"] > SC.GOLDEN_TARGETS).any() or S < 19      # the 19x19 sample holds a table cut by max_targets
