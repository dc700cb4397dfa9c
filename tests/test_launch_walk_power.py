"""The power of tests/test_gpu_capped_launches.py, shown without a GPU: for every launch geometry that module runs, its row count and
its index list notice every fault switch of tests/launch_walk.py that a launch of such blocks can hold -- and the switches it
cannot hold (a partial block or a lone half-wave in a launch of one-row blocks) change nothing there, which is asserted too, not
assumed.  The conditions are the ones the row counts were chosen for: three trips, a partial last block, an index whose entry one
trip later names another record, an entry out of range in every trip, and nothing written behind n."""
import numpy as np
import pytest

from tests import launch_walk as W


def _case_sets():
    """{name: {S: R}}: the number of records of each case set the GPU module lists through an index"""
    from tests import keys_model, race_cases, solve_cases, tactics_cases
    return {"keys": {S: len(keys_model.case_records(S)[1]) for S in (5, 19)},
            "tactics": {S: len(tactics_cases.case_records(S)[1]) for S in (5, 19)},
            "solve": {S: len(solve_cases.case_records(S)[1]) for S in (5, 19)},
            "race": {S: len(race_cases.case_records(S)[1]) for S in (5, 19)}}


@pytest.mark.parametrize("what", ["keys", "tactics", "solve", "race"])
def test_row_counts_and_index_lists_notice_every_switch(what):
    g = W.KEYS if what == "keys" else W.READER
    n, cap, rpb = g["n"], g["cap_rows"], g["rows_per_block"]
    # three trips, the last one short; where a block holds several rows the last block is partial (keys: 3 of 8)
    assert 2 * cap < n < 3 * cap
    assert rpb == 1 or n % rpb != 0
    if what == "keys":
        assert n % rpb == 3 and n % 2 == 1
    else:
        assert n - 2 * cap == 2                                      # rows 131 070 and 131 071 are the third trip
    for S, R0 in _case_sets()[what].items():
        R = W.listed(R0, cap)                                        # a set of 32 records is listed without its last one
        assert R > 4 and R0 - R == (1 if R0 == 32 else 0)
        index = W.wrapped_index(n, cap, R).astype(np.int64)
        oor = (index < 0) | (index >= R)
        assert set(index[oor].tolist()) == set(W.out_of_range(R))
        # a row and its twin one trip later name different records unless both are out of range: iff (cap + 1) % R != 0
        assert (cap + 1) % R != 0, (what, S, R)
        a, b = index[:n - cap], index[cap:]
        assert ((a != b) | (oor[:n - cap] & oor[cap:])).all()
        assert (W.record_of(a, R) != W.record_of(b, R))[~(oor[:n - cap] & oor[cap:])].all()
        assert rpb % R != 0                                          # short_stride: rows_per_block rows earlier is another record
        for k in range(3):
            trip = oor[k * cap:min(n, (k + 1) * cap)]
            assert trip.any() and not trip.all(), (what, S, k)
        good = W.simulate(n, index, R, cap, rpb)
        assert (good[:n] != W.FILL).all() and (good[n:] == W.FILL).all() and len(good) == n + 2
        for fault in W.FAULTS:
            bad = W.simulate(n, index, R, cap, rpb, fault)
            assert (bad[n:] == W.FILL).all()
            if W.applies(fault, rpb):
                differ = np.flatnonzero(bad != good)
                assert len(differ) > 0, (what, S, fault)
                if fault in ("one_trip", "stale_trip"):              # every row behind the first trip shows it but the pairs out of range
                    assert len(differ) >= (n - cap) - 2 * (n // W.EVERY + 1), (what, S, fault, len(differ))
            else:
                assert np.array_equal(bad, good), (what, S, fault)


@pytest.mark.parametrize("S", [5, 19])
def test_secure_row_counts_notice_every_switch(S):
    """k_secure with one workgroup per pair of candidates: n * ch units behind a cap of 1 << 24, so a ROW can straddle the cap.
    The row count puts one row astride it and at least 5 000 rows wholly behind it; every unit of the second trip names another
    record than its twin one trip earlier (or both are out of range); one_trip, short_stride and stale_trip each change entries
    of the row astride the cap and of the whole rows behind it, and nothing before the cap.  A launch of one-unit blocks cannot
    hold a partial block or a lone half-wave."""
    from tests import secure_cases
    ch, n, astride, first_whole, k0 = W.secure_geometry(S)
    cap = W.SECURE_CAP
    assert ch == (S * S + 1) // 2 and astride * ch < cap < first_whole * ch and 0 < k0 < ch and cap == astride * ch + k0
    assert (astride, k0) == {5: (1290555, 1), 19: (92691, 145)}[S]
    assert n - first_whole >= 5000 and n * ch < 2 * cap              # 5 000 whole rows in the second trip, and no third trip
    assert n * S * S * 8 < 300 << 20                                 # the table: under 300 MB
    R0 = len(secure_cases.case_records(S)[1])
    R = W.secure_listed(R0, first_whole)
    assert R > 4 and R0 - R == (1 if S == 5 else 0) and all((first_whole + d) % R for d in (-1, 0, 1))
    index = W.wrapped_index(n, first_whole, R)
    rec = W.record_of(index, R)
    oor = rec == R
    assert oor[n - 1] and oor[:astride].any() and oor[first_whole:].any() and not oor[astride]
    # every unit behind the cap and its twin one trip earlier
    u = np.arange(cap, n * ch, dtype=np.int64)
    a, b = rec[u // ch], rec[(u - cap) // ch]
    assert ((a != b) | ((a == R) & (b == R))).all()
    first = astride - 2                                              # two rows of the first trip, the row astride, everything behind
    good = W.secure_entries(S, index, R, first=first)
    assert (good[:n - first] != W.FILL).all() and (good[n - first:] == W.FILL).all() and good.shape == (n - first + 2, ch)
    assert np.array_equal(good[:n - first], rec[first:n, None] * ch + np.arange(ch)[None, :])
    for fault in W.FAULTS:
        bad = W.secure_entries(S, index, R, fault, first=first)
        assert (bad[n - first:] == W.FILL).all()
        rows = np.flatnonzero((bad != good).any(axis=1)) + first
        if not W.applies(fault, 1):
            assert len(rows) == 0, (S, fault)
            continue
        assert len(rows) > 0 and rows[0] == astride, (S, fault, rows[:4])
        # the row astride the cap: its pairs below k0 are right, the rest wrong
        assert np.array_equal(bad[2, :k0], good[2, :k0]) and (bad[2, k0:] != good[2, k0:]).all(), (S, fault)
        whole = np.setdiff1d(np.arange(first_whole, n), rows)
        if fault == "short_stride":                                  # the unit before: the neighbouring pair, of the row before for pair 0
            assert len(whole) == 0
        else:                                                        # one_trip / stale_trip: all but the rows out of range themselves
            assert len(whole) <= n // W.EVERY + 1 and (oor[whole] | (fault == "stale_trip")).all(), (S, fault, len(whole))


def test_rollout_start_cases_notice_every_switch():
    """k_rollout_start walks one word or one ownership cell per thread.  Case (b) copies three trips of words, (a) and (c) end in a
    partial block, (a) is the only one whose walk is longer than its record words; a cell only ever receives a zero, so a cell
    shows nothing but that it was not written"""
    seen_words, seen_cells = set(), set()
    can = [f for f in W.FAULTS if W.applies(f, W.START_BLOCK) and f != "lone_half"]      # a thread per row: no half-wave of rows
    assert can == ["one_trip", "short_stride", "stale_trip", "tail_dropped"]
    for name, (S, n_src, per_src, cap_src) in sorted(W.START_CASES.items()):
        RW, N, R = 16 * ((S * S + 31) // 32), S * S, W.START_SOURCES
        words, own_n = n_src * per_src * RW, n_src * N
        assert (words, own_n) == {"a": (688000, 1075000), "b": (2111488, 25775), "c": (1152384, 1083361)}[name]
        assert (cap_src + 1) % R != 0 and cap_src == int(round(W.START_CAP / (RW * per_src)))
        oor_free = W.wrapped_index(n_src, cap_src, R, False).astype(np.int64)    # a source list has no out-of-range convention
        assert oor_free.min() == 0 and oor_free.max() == R - 1
        good = W.start_words(S, n_src, per_src, oor_free, R)
        assert (good[:words] != W.FILL).all() and (good[words:] == W.FILL).all()
        for fault in can:
            bad = W.start_words(S, n_src, per_src, oor_free, R, fault)
            assert (bad[words:] == W.FILL).all()
            if not np.array_equal(bad, good):
                seen_words.add((name, fault))
            if not W.start_cells(S, n_src, per_src, fault).all():
                seen_cells.add((name, fault))
        assert W.start_cells(S, n_src, per_src).all()
        assert W.start_cells(S, n_src, per_src, top_from_words=True).all() == (words >= own_n)
    for fault in can:
        assert any(f == fault for _, f in seen_words), fault
    # three trips of words in (b); partial last blocks in (a) and (c); (a) and (c) zero cells behind the first trip
    assert {("b", "one_trip"), ("b", "short_stride"), ("b", "stale_trip"), ("a", "tail_dropped"), ("c", "tail_dropped"),
            ("c", "one_trip"), ("c", "stale_trip")} <= seen_words
    assert seen_cells == {("a", "one_trip"), ("a", "tail_dropped"), ("b", "tail_dropped"), ("c", "one_trip"), ("c", "tail_dropped")}
    S, n_src, per_src, _ = W.START_CASES["a"]
    left = ~W.start_cells(S, n_src, per_src, top_from_words=True)
    assert left.sum() == 1075000 - 688000 and left[-1] and not left[:688000].any()      # the branch `top = max(words, own_n)`


@pytest.mark.parametrize("S", [5, 19])
def test_rollout_start_sources_must_pass(S):
    """every source of the rollout-start cases leaves its mover without a legal board point (the oracle says so), all of them
    differ, and the wall owns the whole board: a rollout from one ends at its first ply under max_plies = 1 with the area score
    of the source, and no sampling model is needed"""
    from oracle import oracle
    from tests import rollout_model as M
    recs, owner = W.start_sources(S)
    assert len(recs) == W.START_SOURCES and len({r.tobytes() for r in recs}) == len(recs) and set(owner.tolist()) == {1, -1}
    for (b, w, wtp), o in zip(W.start_positions(S), owner):
        board = M.board_of(S, b, w, -1 if wtp else 1)
        assert (oracle.legal_moves(board)[:S * S] != 0).all()
        bo, wo = M.owners(board)
        assert bo.all() == (o == 1) and wo.all() == (o == -1) and not (bo & wo).any()


def test_the_golden_collection_repeats_off_the_trip_length():
    """the end-to-end case repeats the five golden games 80 times: 1 647 records (1 642 entries) per repetition, so a row and its
    twin one trip later are different positions, and 400 games stay under the chunk size"""
    from tests.helpers import load
    z = load("sgf_S19.npz")
    entries = sum(len(z["g%02d_moves" % g]) for g in range(5))
    assert (entries, entries + 5) == (1642, 1647)
    assert 65535 % 1647 == 1302 and 32768 % 1647 == 1475 and 32768 % 1642 != 0 and 65535 % 1642 != 0
    assert 80 * 1647 == 131760 < 1 << 18 and 80 * 1647 > 2 * 65535 and 80 * 1642 > 4 * 32768
