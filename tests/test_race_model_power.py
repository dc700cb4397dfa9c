"""What the capturing-race case set (tests/race_cases.py) reaches, on the CPU: every fault switch of tests/race_model.py is noticed by
a named case (one is inert by construction and shown to be); the verdicts of the textbook races are pinned; no constructed case ends
unknown except the budget and depth cases; and the golden sample tests/test_gpu_race.py enumerates shows all four verdicts -- the
condition that test rests on."""
import numpy as np
import pytest

from tests import race_cases as RC
from tests import race_model as M
from tests.tactics_cases import diagram

S0 = 9                                                               # the smallest size that holds every constructed case
INERT = ("flag_as_stone",)

# fault switch -> (how the case is run, its name): a run whose model output differs with the switch on
NOTICED = {
    "desc_order": ("asked", "tiny_b"), "no_pass": ("asked", "tiny_b"), "no_wait": ("asked", "box_b"), "no_second_order": ("asked", "run_b"),
    "no_inner_chains": ("asked", "nakade_b"), "outside_not_terminal": ("asked", "run_b"), "cap_not_terminal": ("asked", "box_b"),
    "cap_off_by_one": ("asked", "eye_b"), "capture_not_terminal": ("asked", "tiny_b"), "adjacency_only": ("enumerated", "box_b"),
    "shared_miscount": ("asked", "shared_b"), "roles_exchanged": ("asked", "plain_2v1_b"), "shared_counter": ("asked", "plain_2v2_b"),
    "d_always": ("asked", "seki_b"), "outside_region": ("region", "connect_b"), "rules_ignored": ("region", "connect_b"),
    "no_root_ko": ("region", "ko_w"), "ko_wrong_side": ("region", "ko_w"), "padding_read": ("enumerated", "tiny_b"),
}


def _one(mode, name, fault=None, rules=1):
    """the model's table of one named case"""
    names, recs, ask, region, has = RC.case_records(S0)
    k = names.index(name)
    kw = dict(rules=rules, max_libs=RC.MAX_LIBS, max_region=RC.MAX_REGION, max_nodes=RC.MAX_NODES, fault=fault)
    if mode == "asked":
        kw["ask"] = ask[k:k + 1]
    elif mode == "region":
        kw["ask"], kw["region"] = ask[k:k + 1], region[k:k + 1]
    m = M.race(S0, recs[k:k + 1], **kw)
    return int(m["n_pairs"][0]), m["rows"][0].tolist(), m["regions"][0].tolist()


def test_every_fault_switch_has_a_case():
    assert sorted(NOTICED) + sorted(INERT) == sorted(set(M.FAULTS) - set(INERT)) + sorted(INERT) and len(M.FAULTS) == len(NOTICED) + len(INERT)


@pytest.mark.parametrize("fault", sorted(NOTICED))
def test_fault_is_noticed(fault):
    mode, name = NOTICED[fault]
    assert _one(mode, name) != _one(mode, name, fault), (fault, mode, name)


@pytest.mark.parametrize("S", M.SIZES)
def test_the_flag_switch_is_inert(S):
    """flag_as_stone (tests/race_model.py argues why): a lone black stone a padding row away from the board changes nothing"""
    names, recs, ask, region, has = RC.case_records(S)
    for rec, pq in zip(recs, ask):
        for a in (None, pq):
            assert M.pair_table(S, rec, a, None, RC.MAX_LIBS, RC.MAX_REGION) == M.pair_table(S, rec, a, None, RC.MAX_LIBS, RC.MAX_REGION, "flag_as_stone")


# the issue's table at 9x9: rules = 1, max_libs 4, black to move and white to move
TABLE = {"plain_2v2": ([2, 4, 2, 2, 0], ("unsettled", "unsettled")), "plain_2v1": ([2, 4, 2, 1, 0], ("safe", "caught")),
         "shared": ([2, 5, 2, 2, 1], ("unsettled", "unsettled")), "seki": ([1, 4, 2, 2, 2], ("safe", "safe")),
         "eye": ([1, 4, 3, 2, 2], ("safe", "caught"))}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_textbook_races(name):
    rows, pq = RC.TABLE[name]
    b, w = diagram(9, rows)
    for wtp in (False, True):
        rec = M.build_record(9, b, w, wtp)
        asked = M.race(9, rec[None], ask=[pq], rules=1, max_libs=4)["rows"][0]
        listed = M.race(9, rec[None], rules=1, max_libs=4)["rows"][0]
        assert len(asked) == 1 and asked[0, :5].tolist() == TABLE[name][0] and M.verdicts(asked[0]) == TABLE[name][1], (name, asked.tolist())
        assert asked[0].tolist() in listed.tolist(), (name, "enumerated")
        if name == "seki":
            assert asked[0, 12:].tolist() == [3, 0, 3, 0] and asked[0, 8:12].tolist() == [-1, -1, -1, -1]


def test_the_seki_is_safe_for_both_without_a_move():
    """either approach is a self-atari that the defender answers by capturing the attacker's racer: three nodes, no move to report"""
    _, rows, _ = _one("asked", "seki_b")
    assert M.verdicts(rows[0]) == ("safe", "safe") and rows[0][8:] == [-1, -1, -1, -1, 3, 0, 3, 0]


def test_verdicts_of_the_other_named_cases():
    """tiny: black has one liberty against two and is caught whoever moves; box: white catches black from the shared centre point and
    black, moving first, saves itself; white is safe; run: the black stone in atari saves itself by capturing the corner stone; nakade: the capture inside the eye does not save
    black; connect: caught under rules = 0, unsettled at the connecting point under rules = 1; the ko: white to play may not retake;
    open and the four ways to ask for no pair"""
    names = RC.case_records(S0)[0]
    asked = {n: RC.asked_model(S0, 1)["rows"][i][0].tolist() for i, n in enumerate(names)}
    pick, reg = RC.region_model(S0, 1)
    given = {names[k]: reg["rows"][i][0].tolist() for i, k in enumerate(pick)}
    given0 = {names[k]: RC.region_model(S0, 0)[1]["rows"][i][0].tolist() for i, k in enumerate(pick)}
    assert M.verdicts(asked["tiny_b"]) == M.verdicts(asked["tiny_w"]) == ("caught", "safe") and asked["tiny_b"][:6] == [1, 2, 1, 2, 0, 5]
    P = lambda x, y: y * S0 + x                                                          # noqa: E731
    assert M.verdicts(asked["box_b"]) == ("unsettled", "safe") and asked["box_b"][:6] == [P(0, 1), P(2, 1), 3, 3, 1, 7]
    assert asked["box_b"][8:12] == [P(1, 1), P(1, 0), -1, -1]
    assert M.verdicts(asked["run_b"])[0] == "unsettled" and asked["run_b"][9] == P(0, 1)
    assert M.verdicts(asked["nakade_b"]) == ("caught", "safe")
    assert M.verdicts(given["connect_b"]) == ("unsettled", "safe") and given["connect_b"][8:10] == [4, 4]
    assert M.verdicts(given0["connect_b"]) == ("caught", "safe")
    assert M.verdicts(given["ko_b"])[0] == "unsettled" and M.verdicts(given["ko_w"])[0] == "safe"
    assert M.verdicts(asked["open_b"]) == ("open", "open") and asked["open_b"][8:] == [-1, -1, -1, -1, 0, 0, 0, 0]
    for n in ("empty_point_b", "point_n_w", "negative_b", "one_colour_w"):
        assert asked[n] == M.NO_PAIR_ROW, n


@pytest.mark.parametrize("S", M.SIZES)
def test_no_constructed_case_ends_unknown(S):
    """asked, enumerated and in the given regions, for both rule sets; the budget and depth cases are run apart"""
    for rules in (1, 0):
        for m in (RC.asked_model(S, rules), RC.enumerated_model(S, rules), RC.region_model(S, rules)[1]):
            for rows in m["rows"]:
                unknown = (M.A_UNKNOWN | M.D_UNKNOWN) * (1 | 1 << M.WHITE_SHIFT)
                assert not (rows[:, 6] & unknown).any(), (S, rules, rows.tolist())


def test_budget_and_depth_cases_end_unknown():
    names, recs, ask, region, has = RC.case_records(S0)
    k = names.index("run_b")
    full = RC.asked_model(S0, 1)["rows"][k][0]
    nodes = int(full[12])
    assert nodes > 100
    kw = dict(ask=ask[k:k + 1], max_libs=RC.MAX_LIBS, max_region=RC.MAX_REGION)
    less = M.race(S0, recs[k:k + 1], max_nodes=nodes - 1, **kw)["rows"][0][0]
    same = M.race(S0, recs[k:k + 1], max_nodes=nodes, **kw)["rows"][0][0]
    black = [8, 9, 12, 13]                                           # the white racer's queries need more and end unknown in both
    assert less[6] & 255 == M.A_UNKNOWN and less[12] == nodes and less[8] == -1 and less[13] == 0
    assert same[6] & 255 == full[6] & 255 and same[black].tolist() == full[black].tolist()
    deep = RC.deep_model()
    row = deep["rows"][0][0]
    assert row[6] & M.A_UNKNOWN and row[12] == 92 and deep["depths"][0][0, 0] == M.MAX_DEPTH
    assert row[6] & (M.A_UNKNOWN << M.WHITE_SHIFT) and row[14] == RC.DEEP_NODES + 1


def test_golden_sample_shows_every_verdict():
    """what tests/test_gpu_race.py::test_golden_sample_enumerated rests on: an all-`unknown` reader cannot pass there"""
    seen, pairs = set(), 0
    for S in M.SIZES:
        m = RC.golden_model(S)
        pairs += int(m["n_pairs"].sum())
        for rows in m["rows"]:
            for row in rows:
                seen.update(M.verdicts(row))
    assert seen == {"safe", "unsettled", "caught", "unknown"} and pairs >= 100, (seen, pairs)
