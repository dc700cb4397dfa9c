"""CPU: the model of the influence map (tests/influence_model.py) says what include/sgo.h states -- the pinned facts of the
definition, a second formulation on numpy arrays that agrees with it on every colouring of a 3x3 corner and on a seeded sample, the
properties the map must have -- and every fault switch of the model changes a compared value of a named case of
tests/influence_cases.py, so a green run of tests/test_gpu_influence.py means something.  No switch is inert: every one has a
position that shows it."""
import itertools

import numpy as np
import pytest

from tests import influence_cases as IC
from tests import influence_model as M

# fault -> [(board size, case name, parameter triple)]: the cases whose compared values the switch changes
NOTICED_BY = {
    "offboard_erodes": [(5, "lone_centre_sb", (5, 10, 21))],
    "padding_rows": [(5, "last_lines_sb", (5, 10, 21)), (19, "last_lines_cw", (4, 0, 0))],
    "column_wrap": [(7, "right_edge_sb", (4, 0, 0))],
    "gauss_seidel": [(5, "lone_centre_sb", (1, 0, 1))],
    "dilate_ignores_opponent": [(5, "contact_sb", (4, 0, 0))],
    "dilate_counts_zero": [(5, "lone_centre_sb", (1, 0, 1))],
    "erode_opposite_only": [(5, "lone_centre_sb", (1, 0, 1))],
    "erode_no_clamp": [(5, "corners_sb", (5, 10, 21))],
    "flag_as_stone": [(5, "empty_cw", (4, 0, 0))],
    "dead_ignored": [(5, "dead_inside_sb", (0, 0, 0))],
    "dead_on_empty": [(5, "dead_inside_sb", (0, 0, 0))],
    "lifted_counted_live": [(5, "dead_inside_cw", (0, 0, 0))],
    "lifted_not_territory": [(5, "dead_inside_sb", (5, 10, 21))],
    # erode_moyo == 0 (the dilated map itself must be read) and in the middle of the schedule
    "moyo_late": [(5, "lone_centre_sb", (1, 0, 1)), (5, "contact_sb", (5, 10, 21))],
    # erode_moyo == erode_terr (the checkpoint is the last step) and in the middle of the schedule
    "moyo_early": [(7, "contact_sb", (8, 31, 31)), (5, "right_edge_sb", (5, 10, 21))],
    "moyo_zero_missed": [(5, "lone_centre_sb", (1, 0, 1))],
    "territory_holds_stones": [(5, "lone_centre_sb", (0, 0, 0))],
}


def _row(S, name, triple, fault=None):
    names, recs, dead = IC.case_records(S)
    i = names.index(name)
    m = IC.case_model(S, triple) if fault is None else M.influence(S, recs[i:i + 1], None, dead[i:i + 1], *triple, fault=fault)
    j = i if fault is None else 0
    return m["values"][j], m["sets"][j], m["counts"][j]


@pytest.mark.parametrize("fault", sorted(NOTICED_BY))
def test_fault_switch_changes_a_named_case(fault):
    for S, name, triple in NOTICED_BY[fault]:
        good, bad = _row(S, name, triple), _row(S, name, triple, fault)
        assert not all(np.array_equal(g, b) for g, b in zip(good, bad)), (fault, S, name, triple)


def test_every_switch_is_shown():
    assert set(M.FAULTS) == set(NOTICED_BY)


# ---- the pinned facts of the definition -------------------------------------------------------------------------------------------
def test_pinned_facts():
    for S in (7, 9, 13, 19):
        m = M.bouzy(S, [(S // 2) * S + S // 2], [])
        assert m["sets"][0] == [] and m["sets"][1] == [] and m["counts"][6] == S * S - 1, S
    m = M.bouzy(5, [12], [])
    assert m["sets"][0] == [a for a in range(25) if a != 12] and m["counts"] == [24, 0, 24, 0, 1, 0, 0, 25]
    assert M.bouzy(5, [12], [], fault="offboard_erodes")["counts"][0] == 0
    m = M.bouzy(19, [2 * 19 + 3], [])
    assert m["counts"][0] == 4 and m["counts"][2] == 18
    assert M.bouzy(19, [3 * 19 + 3], [])["counts"][0] == 0
    v = np.array(M.bouzy(9, [2 * 9 + 2], [6 * 9 + 6])["values"]).reshape(9, 9)
    want = np.zeros((9, 9), int)
    want[0, :2], want[1, :3], want[2, :3] = (4, 7), (7, 12, 10), (0, 10, 134)
    assert np.array_equal(v, want - want[::-1, ::-1])
    full = M.bouzy(9, range(81), [], (), 8, 0, 0)
    assert max(full["values"]) == 160 and min(full["values"]) == 128 + 2 * 8
    # nothing erodes a full board: no on-board neighbour is <= 0 and the missing ones do not count
    assert M.bouzy(9, range(81), [], (), 8, 31, 31)["values"] == full["values"]


# ---- a second formulation: whole arrays, padded shifts, the on-board mask as an array ----------------------------------------------
def array_maps(stones, dilate, erode_moyo, erode_terr):
    """stones int [B, S, S] (+1 / -1 / 0) -> (territory map, moyo map) int [B, S, S]"""
    B, S, _ = stones.shape
    on = np.pad(np.ones((S, S), bool), 1)                     # the board inside a frame of points that do not exist

    def around(a):                                            # the four shifted copies of a framed array, and whether that neighbour exists
        f = np.pad(a, ((0, 0), (1, 1), (1, 1)))
        cut = lambda dy, dx: (f[:, 1 + dy:1 + dy + S, 1 + dx:1 + dx + S], on[1 + dy:1 + dy + S, 1 + dx:1 + dx + S])   # noqa: E731
        return [cut(-1, 0), cut(1, 0), cut(0, -1), cut(0, 1)]

    v = stones.astype(np.int64) * 128
    for _ in range(dilate):
        pos = sum(((n > 0) & e).astype(np.int64) for n, e in around(v))
        neg = sum(((n < 0) & e).astype(np.int64) for n, e in around(v))
        v = v + np.where((v >= 0) & (neg == 0), pos, 0) - np.where((v <= 0) & (pos == 0), neg, 0)
    moyo = v
    for step in range(erode_terr):
        le = sum(((n <= 0) & e).astype(np.int64) for n, e in around(v))
        ge = sum(((n >= 0) & e).astype(np.int64) for n, e in around(v))
        v = np.where(v > 0, np.maximum(v - le, 0), np.where(v < 0, np.minimum(v + ge, 0), 0))
        if step + 1 == erode_moyo:
            moyo = v
    return v, moyo


def _agree(S, stones, triple):
    terr, moyo = array_maps(stones, *triple)
    for k in range(len(stones)):
        flat = stones[k].reshape(-1)
        m = M.bouzy(S, np.flatnonzero(flat > 0).tolist(), np.flatnonzero(flat < 0).tolist(), (), *triple)
        assert m["values"] == terr[k].reshape(-1).tolist(), (S, triple, flat.tolist())
        empty = flat == 0
        for j, (mp, sign) in enumerate(((terr, 1), (terr, -1), (moyo, 1), (moyo, -1))):
            assert m["sets"][j] == np.flatnonzero(empty & (mp[k].reshape(-1) * sign > 0)).tolist(), (S, triple, j, flat.tolist())


@pytest.mark.parametrize("triple", M.TRIPLES)
def test_array_formulation_on_every_3x3_corner_colouring(triple):
    """all 19 683 colourings of the 3x3 corner of the 5x5 board"""
    stones = np.zeros((3 ** 9, 5, 5), np.int64)
    for k, cells in enumerate(itertools.product((0, 1, -1), repeat=9)):
        stones[k, :3, :3] = np.array(cells).reshape(3, 3)
    _agree(5, stones, triple)


def test_array_formulation_on_a_seeded_9x9_sample():
    rng = np.random.RandomState(99)
    for triple in M.TRIPLES:
        stones = rng.choice([0, 0, 0, 1, -1], size=(12, 9, 9), p=None).astype(np.int64)
        stones[0] = 0
        stones[1, rng.randint(9), :] = 1
        _agree(9, stones, triple)


# ---- properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", M.SIZES)
def test_properties_on_seeded_positions(S):
    """the eight tables of sgo_sym_lut permute the outputs; swapping the colours negates the values and swaps the sets; territory
    lies inside moyo; a live stone keeps its sign at erosion 31; neutral and margin are what the header defines; the flag and bits
    >= N of `dead` change nothing"""
    from tests.keys_model import luts
    N = S * S
    L = luts(S)
    rng = np.random.RandomState(700 + S)
    for trial in range(4 if S <= 9 else 2):
        cells = rng.choice([0, 1, -1], size=N, p=[0.7, 0.15, 0.15])
        b, w = np.flatnonzero(cells > 0).tolist(), np.flatnonzero(cells < 0).tolist()
        dead = [a for a in b + w if rng.rand() < 0.1]
        for triple in ((5, 10, 21), (8, 31, 31) if trial == 0 else (4, 0, 0)):
            base = M.bouzy(S, b, w, dead, *triple)
            tb, tw, yb, yw = (set(s) for s in base["sets"])
            live_b, live_w = set(b) - set(dead), set(w) - set(dead)
            assert tb <= yb and tw <= yw and not (tb | tw) & (live_b | live_w)
            assert all(base["values"][a] > 0 for a in live_b) and all(base["values"][a] < 0 for a in live_w)
            c = base["counts"]
            assert c[:6] == [len(tb), len(tw), len(yb), len(yw), len(live_b), len(live_w)]
            assert c[6] == N - len(live_b) - len(live_w) - len(tb) - len(tw) and c[7] == (len(live_b) + len(tb)) - (len(live_w) + len(tw))
            assert max(abs(x) for x in base["values"]) <= 160
            sw = M.bouzy(S, w, b, dead, *triple)
            assert sw["values"] == [-x for x in base["values"]]
            assert sw["sets"] == (base["sets"][1], base["sets"][0], base["sets"][3], base["sets"][2])
            assert sw["counts"] == [c[1], c[0], c[3], c[2], c[5], c[4], c[6], -c[7]]
            assert M.bouzy(S, b, w, dead + [N, N + 5], *triple, flag=True) == base
            for k in range(8) if S <= 9 else (1 + trial, 6):
                t = lambda s: sorted(int(L[k, a]) for a in s)                            # noqa: E731
                moved = M.bouzy(S, t(b), t(w), t(dead), *triple)
                assert moved["counts"] == c, (S, k)
                assert all(moved["values"][int(L[k, a])] == base["values"][a] for a in range(N)), (S, k)
                assert moved["sets"] == tuple(t(s) for s in base["sets"]), (S, k)


def test_case_records_carry_what_they_name():
    """the record builder and the reader agree: every case reads back as drawn, whatever the flag and the padding hold; bits a >= N
    of the sets are zero"""
    for S in M.SIZES:
        names, recs, dead = IC.case_records(S)
        for i, (name, b, w, wtp, d) in enumerate(IC.case_points(S)):
            assert M.record_stones(S, recs[i]) == (sorted(b), sorted(w), wtp), name
        N, NW = S * S, (S * S + 31) // 32
        top = np.uint32(0xFFFFFFFF) << np.uint32(N & 31) if N & 31 else np.uint32(0)
        for triple in ((5, 10, 21), (0, 0, 0)):
            assert not (IC.case_model(S, triple)["sets"][:, :, NW - 1] & top).any()
        assert dead[names.index("dead_inside_sb"), NW - 1] >> 31                         # the stray bit beside the flag's place
