"""No GPU: what the cases of tests/rollout_cases.py (run on the device by tests/test_gpu_rollout_step.py) can catch and reach.

 * power: every fault of rollout_model.FAULTS -- each the kind of slip k_rollout_step could hold -- changes at least one value
   the GPU test compares (an action shows in the record written, so: record words, survivors, results) in the group of cases
   named in CATCHERS;
 * coverage: conditions on the cases themselves -- the depth of the scoring fill on the end positions, regions reached by both
   colours, every pick boundary with both outcomes, the largest total, every special value on a legal point;
 * builder self-checks and a few guard vectors."""
import numpy as np
import pytest

from oracle import oracle
from tests import rollout_cases as RC
from tests import rollout_model as M
from tests import rule_shapes as rs

# fault -> the cases that catch it
CATCHERS = {
    "pick_ge": [("boundaries", 5, "dense"), ("boundaries", 19, "empty")],        # t on a prefix sum: the pick is the NEXT point
    "row_boundary_lt": [("boundaries", 13, "dense"), ("boundaries", 5, "empty")],  # ... across a row end / an empty row
    "no_plus_one": [("specials", 5, "empty"), ("boundaries", 13, "ko")],
    "round_not_floor": [("boundaries", 13, "empty")],                            # the 'below' encoding
    "no_clamp_hi": [("specials", 13, "dense"), ("max_total",)],
    "nan_as_one": [("specials", 19, "empty")],
    "neg_as_abs": [("specials", 5, "dense")],
    "scan_wraps_28": [("max_total",)],
    "fill_capped": [("probes", 5, False), ("neighbours", 7, "DED")],
    "owner_no_exclusion": [("probes", 5, False), ("probes", 5, True)],
    "seed_unmasked": [("probes", 5, False)],
    "history_from_out": [("probes", 5, False), ("chains", 5)],
    "meta_not_flipped": [("probes", 5, True), ("chains", 5)],
}
RECORD_FAULTS = ("history_from_out", "meta_not_flipped")


def _changed(key, fault):
    """How many compared values of a case the fault changes: (record words, survivor flags, result entries)."""
    c, e = RC.case(key), RC.expected(key)
    if fault in RECORD_FAULTS:
        prev = c.records[np.repeat(c.index, c.per_src)]
        return int((M.expected_records(prev, e.pair[0], fault) != M.expected_records(prev, e.pair[0])).sum()), 0, 0
    f = RC.expect(c, fault)
    return (int((f.pair != e.pair).sum()), int((f.live_after != e.live_after).sum()),
            int((f.black_own != e.black_own).sum() + (f.white_own != e.white_own).sum() + (f.sums != e.sums).sum()))


def test_every_fault_has_a_catcher():
    assert set(CATCHERS) == set(M.FAULTS) and len(M.FAULTS) == 13


@pytest.mark.parametrize("fault", M.FAULTS)
def test_faults_change_expected_values(fault):
    for key in CATCHERS[fault]:
        words, lists, results = _changed(key, fault)
        print("%-18s %-28s changes %6d record words, %4d survivor flags, %6d result entries" % (fault, key, words, lists, results))
        assert words + lists + results > 0, key
        if fault in M.FILL_FAULTS:
            assert results > 0 and words == 0                       # only the score can show a wrong fill


def test_capped_fill_passes_what_the_whole_game_cases_reach():
    """FILL_CAP is the deepest fill the end positions of tests/test_gpu_rollout.py's sources were measured to need; a fill
    that shallow is untouched by the cap, one trip more is not."""
    real = np.zeros((5, 5), dtype=np.int8)
    real[0, 0], real[4, 4] = 1, -1
    assert M.owners_rows_real(real)[2] <= M.FILL_CAP
    a, b = M.owners_rows_real(real), M.owners_rows_real(real, "fill_capped")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------- coverage conditions
@pytest.mark.parametrize("S", RC.SIZES)
def test_fill_depth_and_shared_regions_on_the_end_positions(S):
    """The scoring fill of the probes' END positions needs at least S*S/2 - S trips (7, 17, 31, 71, 161), measured with
    rule_shapes.flood; regions reached by both colours occur."""
    p, a, trips = RC.deepest_probe(S)
    e = RC.expected(("probes", S, False))
    print("S=%d: %d + %d probes, %d chains; deepest scoring fill %d trips (position %s, point %d); %d end positions with a region "
          "of both colours" % (S, len(RC.probe_items(S)[0]), len(RC.probe_items(S)[1]), RC.case(("chains", S)).n_total, trips,
                               rs.load_shapes(S).names[p], a, int(e.both.sum())))
    assert trips >= S * S / 2 - S
    assert e.both.any() and RC.expected(("chains", S)).both.any()
    n_pass = len(set(p for p, _ in RC.probe_items(S)[1]))
    assert 28 <= n_pass <= 39 and (RC.expected(("probes", S, True)).plies == 2).all()
    # the neighbours' deep one is that probe
    c = RC.case(("neighbours", S, "DED"))
    assert RC.fill_depth(RC.expected(("neighbours", S, "DED")).end_real[0], S) == trips and c.n_total == 3
    e = RC.expected(("neighbours", S, "DED"))
    assert RC.fill_depth(e.end_real[1], S) == 1 and e.action[0].tolist() == [a, S * S, a]      # the quiet one passes


def _boundary_figures(c, g):
    """(legal list, weights over it, t, prefix sums) of row g of a boundary case, from the row itself"""
    L = RC.legal_list(c.boards)
    row = oracle.sym_policy_inverse(c.S, c.sym[0], c.rows0[g]) if c.sym[0] else c.rows0[g]
    w = M.weights_arr(row[L])
    t = (M.draw(c.seed, g, 0) * int(w.sum())) >> 32
    return L, w, t, np.cumsum(w)


@pytest.mark.parametrize("S", RC.BOUNDARY_SIZES)
def test_pick_boundaries_are_present_and_exact(S):
    """Builder self-check and coverage in one pass over every row: weights in range, the sum exact, the prefix sum through L[j]
    exactly t + 1 or t, the model's pick the point the row was built for; every kind with both outcomes; both encodings."""
    seen = set()
    for where in ("empty", "dense", "ko"):
        c, e = RC.case(("boundaries", S, where)), RC.expected(("boundaries", S, where))
        for g, (kind, hit, cls, enc, j, T, want) in enumerate(c.meta):
            L, w, t, cum = _boundary_figures(c, g)
            assert w.min() >= 1 and w.max() <= RC.W_MAX and int(w.sum()) == T
            assert int(cum[j]) == (t + 1 if hit else t) and want == (L[j] if hit else L[j + 1]) == int(e.action[0, g])
            y0, y1 = L[j] // S, L[j + 1] // S
            assert {"first_two": j == 0, "last_two": j == len(L) - 2, "row_end": y1 == y0 + 1, "gap_row": y1 > y0 + 1,
                    "t0": t == 0 and want == L[0], "t_last": t == T - 1 and want == L[-1]}[kind]
            seen.add((kind, hit))
            seen.add(("total", cls, enc))
    assert all((kind, hit) in seen for kind in RC.KINDS[:4] for hit in (True, False))
    assert ("t0", True) in seen and ("t_last", False) in seen
    assert all(("total", cls, enc) in seen for cls in ("small", "mid", "big") for enc in ("exact", "below", "mixed")[:2 if cls == "small" else 3])
    ys = set(a // S for a in RC.legal_list(RC.boundary_positions(S)["dense"]))
    assert any(y not in ys and y - 1 in ys for y in range(min(ys), max(ys)))        # a row without a legal point in between
    b = RC.boundary_positions(S)["ko"]
    assert ((b[0, :, :, 2] != 0) & (b[0, :, :, 0] == 0)).sum() == 1                    # the ko point


def test_encodings_round_trip():
    w = np.array([1, 2, 3, 517, 1024, (1 << 19) + 12345, 1 << 20, RC.W_MAX], dtype=np.int64)
    for how in ("exact", "below", "mixed"):
        p = RC.encode(w, how)
        assert p.dtype == np.float32 and M.weights(p) == w.tolist()
    assert (RC.encode(w, "below") > RC.encode(w, "exact")).all()
    assert M.weights_arr(RC.encode(w, "below"), "round_not_floor").tolist() == (w + 1).tolist()[:-1] + [RC.W_MAX]
    assert RC.boundary_weights([3, 4, 9], 0x80000000, 0, 10, True) == [6, 2, 2]       # t = 5: the prefix through L[0] is 6
    assert RC.boundary_weights([3, 4, 9], 0x80000000, 0, 10, False) == [5, 3, 2]
    assert RC.boundary_weights([3, 4, 9], 0xFFFFFFFF, 0, 3, True) is None             # t = 2 needs three points in front


def test_largest_total():
    c, e = RC.case(("max_total",)), RC.expected(("max_total",))
    for g in (0, 1, 2, 3, 255):
        w = M.weights_arr(c.rows0[g][:361])
        assert int(w.sum()) == RC.MAX_TOTAL == 361 * ((1 << 20) + 1) and int(np.cumsum(w)[-1]) > 1 << 28
    t = np.array([(M.draw(c.seed, g, 0) * RC.MAX_TOTAL) >> 32 for g in range(c.n_total)])
    assert (t > 1 << 28).sum() > 20 and (e.action[0] == t // RC.W_MAX).all()          # equal weights: the pick is a division


@pytest.mark.parametrize("S", RC.BOUNDARY_SIZES)
def test_special_values_land_on_legal_points(S):
    vals = np.array([v for _, v in RC.VALUES], dtype=np.float32)
    assert len(vals) == 14 and len(set(vals.view(np.uint32).tolist())) == 14
    assert M.weights(vals) == [1, 1, 1, 1, 1, RC.W_MAX, RC.W_MAX, RC.W_MAX, 1 << 20, RC.W_MAX, 2, 1, 1, 1]
    for where in ("empty", "dense"):
        c = RC.case(("specials", S, where))
        L = RC.legal_list(c.boards)
        bits = c.rows0.view(np.uint32)
        for a in (L[0], L[len(L) // 2], L[-1]):
            assert set(bits[:, a].tolist()) == set(vals.view(np.uint32).tolist())       # every value, on this legal point
        pas = c.rows0[:, c.A - 1]
        assert np.isnan(pas[0::2]).all() and np.isinf(pas[1::2]).all()
        assert len(set(RC.expected(("specials", S, where)).action[0].tolist())) > 4


# ---------------------------------------------------------------------------------------------- builder self-checks
def test_symmetry_rows_map_back():
    for S in (13, 19):
        base = RC.case(("boundaries", S, "dense"))
        seen = set()
        for k in range(8):
            c, e = RC.case(("boundaries", S, "dense", k)), RC.expected(("boundaries", S, "dense", k))
            assert np.array_equal(oracle.sym_policy_inverse(S, k, c.rows0).view(np.uint32), base.rows0.view(np.uint32))
            assert np.array_equal(e.action, RC.expected(("boundaries", S, "dense")).action)
            seen.add(c.rows0.tobytes())
        assert len(seen) == 8                                           # the position is asymmetric: eight different tensors


def test_row_form_scoring_equals_the_oracle():
    """owners_rows (the fill the fill faults alter) with no fault = the oracle's owners, on every probe's end position at 5x5
    and on the fixture positions of 9x9."""
    f = rs.load_shapes(5)
    c, e = RC.case(("probes", 5, False)), RC.expected(("probes", 5, False))
    total_b = np.zeros((c.n_src, 25), np.int32)
    for g in range(c.n_total):
        total_b[g] = M.owners_rows_real(e.end_real[g].reshape(5, 5))[0]
    assert np.array_equal(total_b, e.black_own)
    f = rs.load_shapes(9)
    for p in range(0, f.P, 3):
        a, b = M.owners(f.boards[p:p + 1]), M.owners_rows(f.boards[p:p + 1])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_expected_record_and_step_row():
    """One ply by hand: planes 0 / 1 and the to-play bit from the model's board, the history and every spare bit from the
    record read."""
    S, NW = 5, 1
    board = M.board_of(S, [6, 7], [12], to_play=1)
    prev = RC.source_table(board, 9)[0]
    assert prev[0] == (1 << 6 | 1 << 7) and prev[1] & 0x1FFFFFF == 1 << 12 and prev[4:].all()
    row = np.zeros(26, np.float32)
    row[13] = 1.0
    a, new = M.step_row(board, row, M.draw(1, 0, 0))
    assert a == 13 and board[0, 2, 3, 0] == 0 and new[0, 2, 3, 1] == 1 and new[0, 0, 0, 16] == -1
    want = M.expected_record(prev, new)
    assert want[0] == (1 << 6 | 1 << 7 | 1 << 13 | 0x80000000) and want[1] == 1 << 12
    assert np.array_equal(want[2:], prev[:14]) and np.array_equal(want[:2], M.pack_boards(new)[0][:2])
    assert M.expected_record(prev, new, "meta_not_flipped")[0] == want[0] & 0x7FFFFFFF
    assert np.array_equal(M.expected_record(prev, new, "history_from_out")[2:4], want[:2])
    # an occupied point weighs nothing: the draw falls on the floor of 1-weights of the legal points
    row[:] = 0
    row[6] = 1.0
    a, _ = M.step_row(board, row, 0xFFFFFFFF)
    assert a == 24


# ---------------------------------------------------------------------------------------------- guard vectors
GUARD = [(("probes", 5, False), (0, 1, 1000, 2924), (1, 6, 10, 0)),
         (("chains", 5), (0, 7, 365), (11, 6, 20)),
         (("boundaries", 5, "dense"), (0, 1, 2, 191), (0, 22, 0, 22)),
         (("boundaries", 19, "empty"), (0, 5, 1535), (0, 1, 19)),
         (("specials", 13, "dense"), (0, 17, 55), (64, 19, 106)),
         (("max_total",), (0, 128, 255), (96, 161, 13))]


def test_guard_vectors():
    """(case, rollouts, their first actions) as literals: a change to the builder is noticed."""
    got = [(key, gs, tuple(int(RC.expected(key).action[0, g]) for g in gs)) for key, gs, _ in GUARD]
    assert got == GUARD
    assert [int(RC.expected(("chains", 5)).action[2, g]) for g in (0, 7, 365)] == GUARD_CHAIN_PLY3


GUARD_CHAIN_PLY3 = [8, 18, 22]
