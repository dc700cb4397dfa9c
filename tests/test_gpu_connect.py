"""GPU: the connection kernels (include/sgo.h "connections", csrc/sgo_connect.hip) against the model (tests/connect_model.py) word for
word -- n_pairs, table rows, region sets, group map and group counts -- at every board size, for both rule sets, asked and enumerated,
on the case set tests/test_connect_model_power.py shows to notice the model's fault switches (tests/connect_cases.py)."""
import numpy as np
import pytest

from tests import connect_cases as CC
from tests import connect_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG = -1
FILL = 0x3C3C3C3C
FILL16 = 0x3C3C
T = 10                                                               # table rows per position in most calls: no case lists more than 9
KEYS = ("n_pairs", "rows", "regions", "groups", "counts")


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _filled(S, n, max_pairs, dev=None):
    """sentinel-filled outputs for n rows: numpy without a device, torch tensors on it"""
    NW = (S * S + 31) // 32
    if dev is None:
        return (np.full(n, FILL, np.int32), np.full((n, max_pairs, M.W), FILL, np.int32), np.full((n, max_pairs, NW), FILL, np.uint32),
                np.full((n, S * S), FILL16, np.int16), np.full((n, 4), FILL, np.int32))
    import torch
    return (torch.full((n,), FILL, dtype=torch.int32, device=dev), torch.full((n, max_pairs, M.W), FILL, dtype=torch.int32, device=dev),
            torch.full((n, max_pairs, NW), FILL, dtype=torch.int32, device=dev), torch.full((n, S * S), FILL16, dtype=torch.int16, device=dev),
            torch.full((n, 4), FILL, dtype=torch.int32, device=dev))


def _numpy(n_pairs, rows, regions, groups, counts):
    return {"n_pairs": n_pairs.cpu().numpy(), "rows": rows.cpu().numpy(), "regions": regions.cpu().numpy().view(np.uint32),
            "groups": groups.cpu().numpy(), "counts": counts.cpu().numpy()}


def _run(S, records, index=None, ask=None, region=None, rules=1, cut_libs=CC.CUT_LIBS, max_region=CC.MAX_REGION, max_nodes=CC.MAX_NODES,
         max_pairs=T, n=None, n_records=None, pad=2):
    """sgo_connect_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    n = (len(index) if index is not None else len(records)) if n is None else n
    up = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t).view(np.int32)).to(dev)   # noqa: E731
    d_rec, d_idx, d_ask, d_reg = up(records, np.uint32), up(index, np.int32), up(ask, np.int32), up(region, np.uint32)
    out = _filled(S, n + pad, max_pairs, dev)
    rc = lib.sgo_connect_dev(S, n, L.ptr(d_rec), len(records) if n_records is None else n_records, L.ptr(d_idx), L.ptr(d_ask), L.ptr(d_reg),
                             rules, cut_libs, max_region, max_nodes, max_pairs, *([L.ptr(t) for t in out] + [L.stream_ptr()]))
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return _numpy(*out)


def _same(got, want, n, what):
    """n_pairs, every word of the listed rows and region sets, the group map and its counts; everything behind them, and the map and
    counts of a row out of range, are as they were filled"""
    assert got["n_pairs"][:n].tolist() == want["n_pairs"][:n].tolist(), (what, "n_pairs", got["n_pairs"][:n].tolist(), want["n_pairs"][:n].tolist())
    for i in range(n):
        k = len(want["rows"][i])
        assert got["rows"][i, :k].tolist() == want["rows"][i].tolist(), (what, "row", i, got["rows"][i, :k].tolist(), want["rows"][i].tolist())
        assert got["regions"][i, :k].tolist() == want["regions"][i].tolist(), (what, "region", i)
        assert (got["rows"][i, k:] == FILL).all() and (got["regions"][i, k:] == FILL).all(), (what, "rows behind the listed ones", i)
        if want["groups"][i] is None:
            assert (got["groups"][i] == FILL16).all() and (got["counts"][i] == FILL).all(), (what, "map of a row out of range", i)
        else:
            assert got["groups"][i].tolist() == want["groups"][i].tolist(), (what, "groups", i, got["groups"][i].tolist(), want["groups"][i].tolist())
            assert got["counts"][i].tolist() == want["counts"][i].tolist(), (what, "counts", i, got["counts"][i].tolist(), want["counts"][i].tolist())
    assert (got["n_pairs"][n:] == FILL).all() and (got["rows"][n:] == FILL).all() and (got["regions"][n:] == FILL).all(), (what, "rows behind n")
    assert (got["groups"][n:] == FILL16).all() and (got["counts"][n:] == FILL).all(), (what, "maps behind n")


def _indexed(want, index, R):
    """the model's outputs of records 0 .. R - 1 re-listed through an index (out of range: no pairs, no map)"""
    NW = want["regions"][0].shape[1]
    ok = [0 <= r < R for r in index]
    return {"n_pairs": np.array([want["n_pairs"][r] if o else 0 for r, o in zip(index, ok)], np.int32),
            "rows": [want["rows"][r] if o else np.zeros((0, M.W), np.int32) for r, o in zip(index, ok)],
            "regions": [want["regions"][r] if o else np.zeros((0, NW), np.uint32) for r, o in zip(index, ok)],
            "groups": [want["groups"][r] if o else None for r, o in zip(index, ok)],
            "counts": [want["counts"][r] if o else None for r, o in zip(index, ok)]}


@pytest.mark.parametrize("S", M.SIZES)
def test_case_set_word_for_word(S):
    """every constructed position for both sides to move and both rule sets: asked in the default region and enumerated, in order
    without an index list and with an odd number of rows (the last wave's second half idles in k_connect_pairs and k_connect_groups;
    the rows with one pair or three leave the odd half of k_connect_read idle), and through a list that permutes them, repeats some
    and holds entries out of range; asked in the given regions; the host twin"""
    L, lib = _lib()
    names, recs, ask, region, has = CC.case_records(S)
    R = len(recs)
    rng = np.random.RandomState(S)
    index = np.concatenate([rng.permutation(R)[:R - 8], [-1, R, 0, 0, 2 ** 31 - 1, -2 ** 31, R - 1]]).astype(np.int64)
    assert len(index) % 2 == 1 and len(index) <= 64 and R <= 64
    safe = np.clip(index, 0, R - 1)
    for rules in (1, 0):
        want = CC.asked_model(S, rules)
        _same(_run(S, recs, ask=ask, rules=rules), want, R, ("asked", rules))
        _same(_run(S, recs[:R - 1], ask=ask[:R - 1], rules=rules), want, R - 1, ("asked, odd n", rules))
        _same(_run(S, recs, index.astype(np.int32), ask=ask[safe], rules=rules), _indexed(want, index, R), len(index), ("asked, indexed", rules))
        want = CC.enumerated_model(S, rules)
        assert {len(r) for r in want["rows"]} >= {0, 1, 2, 3}
        _same(_run(S, recs, rules=rules), want, R, ("enumerated", rules))
        _same(_run(S, recs, index.astype(np.int32), ask=np.full((len(index), 2), -1), rules=rules), _indexed(want, index, R), len(index),
              ("enumerated through ask = -1, indexed", rules))
        pick, want = CC.region_model(S, rules)
        _same(_run(S, recs, pick.astype(np.int32), ask=ask[pick], region=region[pick], rules=rules), want, len(pick), ("given regions", rules))
        out = _filled(S, R, T)
        assert lib.sgo_connect(S, R, L.ptr(np.ascontiguousarray(recs)), L.ptr(np.ascontiguousarray(ask)), None, rules, CC.CUT_LIBS, CC.MAX_REGION,
                               CC.MAX_NODES, T, *[L.ptr(a) for a in out]) == 0
        _same(dict(zip(KEYS, out)), CC.asked_model(S, rules), R, ("host twin", rules))


@pytest.mark.parametrize("cut_libs", (0, 2))
def test_cut_libs(cut_libs):
    """cut_libs 0: no cutting chain, cutter_atari has no link point and reads open; cut_libs 2: the crosscut's chains are cutting
    chains (enumerated; the asked peep is the budget case below)"""
    S = 7
    names, recs, ask, region, has = CC.case_records(S)
    want = CC.enumerated_model(S, 1, cut_libs=cut_libs)
    _same(_run(S, recs, cut_libs=cut_libs), want, len(recs), ("enumerated", cut_libs))
    if cut_libs == 0:
        k = names.index("cutter_atari_b")
        want = M.connect(S, recs[k:k + 1], ask=ask[k:k + 1], cut_libs=0)
        assert M.verdict(want["rows"][0][0]) == "open" and want["rows"][0][0][4] == 0
        _same(_run(S, recs[k:k + 1], ask=ask[k:k + 1], cut_libs=0), want, 1, "cutter_atari at cut_libs 0")


def test_max_pairs_cuts_the_table_not_the_count():
    """max_pairs = 2 on positions that list up to nine pairs: n_pairs stays, two rows are written, the rows behind them are untouched,
    the group map ties what the written rows tie and flag 1 says the table was cut"""
    S = 7
    names, recs, ask, region, has = CC.case_records(S)
    want = CC.enumerated_model(S, 1, max_pairs=2)
    assert max(want["n_pairs"]) >= 9 and any(c[3] & M.FLAG_CUT_TABLE for c in want["counts"])
    full = CC.enumerated_model(S, 1)
    assert any(a[1] != b[1] for a, b in zip(want["counts"], full["counts"]))   # the cut table leaves a finer partition somewhere
    _same(_run(S, recs, max_pairs=2), want, len(recs), "max_pairs 2")


def test_node_budget_exact_and_one_less():
    """max_nodes equal to the node count of a query decides it; one less ends it unknown with the count at that moment.  The peep
    at cut_libs 2 (nine empty points) does not finish within any budget up to the cap: at 4 096 nodes and at one less it ends
    unknown with one node more than the budget counted"""
    S = 7
    names, recs, ask, region, has = CC.case_records(S)
    k = names.index("diagonal_b")
    full = CC.asked_model(S, 1)["rows"][k][0]
    nodes = int(full[10])
    assert nodes == 145 and M.verdict(full) == "connected"
    for budget in (nodes, nodes - 1):
        want = M.connect(S, recs[k:k + 1], ask=ask[k:k + 1], rules=1, max_nodes=budget)
        assert bool(want["rows"][0][0][6] & M.A_UNKNOWN) == (budget < nodes) and want["rows"][0][0][10] == nodes
        _same(_run(S, recs[k:k + 1], ask=ask[k:k + 1], max_nodes=budget), want, 1, ("budget", budget))
    k = names.index("peep_b")
    for budget in (4096, 4095):
        want = M.connect(S, recs[k:k + 1], ask=ask[k:k + 1], rules=1, cut_libs=2, max_region=9, max_nodes=budget)
        row = want["rows"][0][0]
        assert row[5] == 9 and row[6] == M.A_UNKNOWN and row[10] == budget + 1 and want["counts"][0][3] == M.FLAG_UNDECIDED
        _same(_run(S, recs[k:k + 1], ask=ask[k:k + 1], cut_libs=2, max_region=9, max_nodes=budget), want, 1, ("peep budget", budget))


def test_depth_cap():
    """a query whose first line of play passes depth 80 ends unknown there, after 82 nodes"""
    rec, pq, region = CC.deep_case()
    want = CC.deep_model()
    row = want["rows"][0][0]
    assert row[6] == M.A_UNKNOWN and row[10] == 82 and want["depths"][0][0, 0] == 80
    _same(_run(19, rec[None], ask=[pq], region=region[None], max_region=CC.DEEP_REGION, max_nodes=CC.DEEP_NODES), want, 1, "depth cap")


def test_golden_sample_enumerated():
    """plies of the golden play-outs (and, at 19x19, one position of the golden game records) enumerated at (cut_libs 1, max_region 5,
    max_nodes 128); each of the four read verdicts occurs, so an all-`unknown` reader cannot pass by agreeing with an all-`unknown`
    model, and somewhere a group holds more than one chain"""
    seen, tied = set(), 0
    for S in M.SIZES:
        recs = CC.golden_sample(S)
        assert len(recs) <= 64
        want = CC.golden_model(S)
        got = _run(S, recs, cut_libs=CC.GOLDEN_CUT_LIBS, max_region=CC.GOLDEN_REGION, max_nodes=CC.GOLDEN_NODES, max_pairs=CC.GOLDEN_PAIRS)
        _same(got, want, len(recs), ("golden", S))
        for i in range(len(recs)):
            tied += int(got["counts"][i][0] - got["counts"][i][1])
            for row in got["rows"][i, :min(int(got["n_pairs"][i]), CC.GOLDEN_PAIRS)]:
                seen.add(M.verdict(row))
    assert seen == {"connected", "unsettled", "cut", "unknown"} and tied > 0, (seen, tied)


def test_row_counts_and_bad_arguments():
    """n of 0, 1, 2, 3; n_records bounds the index; the refusals leave the outputs as they were"""
    import torch
    L, lib = _lib()
    S = 7
    names, recs, ask, region, has = CC.case_records(S)
    want = CC.asked_model(S, 1)
    idx = np.array([names.index("diagonal_b"), names.index("jump_w"), names.index("peep_b")], np.int32)
    for n in (0, 1, 2, 3):
        _same(_run(S, recs, idx[:max(n, 1)], ask=ask[idx[:max(n, 1)]], n=n), _indexed(want, idx[:n], len(recs)), n, n)
    k = int(idx[0])
    _same(_run(S, recs, np.array([k, k + 1], np.int32), ask=ask[[k, k + 1]], n_records=k + 1), _indexed(want, [k, -1], len(recs)), 2, "n_records")
    dev = torch.device("cuda", 0)
    d = torch.zeros(1024, dtype=torch.int32, device=dev)
    out = _filled(S, 2, T, dev)
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), kw.get("R", 1), None, None, None, kw.get("rules", 1),   # noqa: E731
                         kw.get("libs", 1), kw.get("region", 6), kw.get("nodes", 64), kw.get("pairs", T), kw.get("o0", P(out[0])),
                         kw.get("o1", P(out[1])), kw.get("o2", P(out[2])), kw.get("o3", P(out[3])), kw.get("o4", P(out[4])), L.stream_ptr()]
    for bad in (dict(S=8), dict(S=0), dict(n=-1), dict(R=-1), dict(rules=2), dict(rules=-1), dict(libs=-1), dict(libs=5), dict(region=0),
                dict(region=33), dict(nodes=0), dict(nodes=32769), dict(pairs=0), dict(pairs=65), dict(rec=None), dict(o0=None), dict(o1=None),
                dict(o2=None), dict(o3=None), dict(o4=None)):
        assert lib.sgo_connect_dev(*args(**bad)) == SGO_ERR_ARG, bad
    torch.cuda.synchronize()
    assert all(bool((t == (FILL16 if t.dtype == torch.int16 else FILL)).all()) for t in out)
    for good in (dict(), dict(libs=0), dict(libs=4), dict(region=1), dict(region=32), dict(nodes=1), dict(nodes=32768), dict(pairs=1)):
        assert lib.sgo_connect_dev(*args(**good)) == 0, good           # the empty board: nothing to list, an all-empty map
    torch.cuda.synchronize()
    assert out[0].tolist() == [0, FILL] and (out[1] == FILL).all() and (out[2] == FILL).all()
    assert (out[3][0] == -1).all() and (out[3][1] == FILL16).all() and out[4].tolist() == [[0, 0, 0, 0], [FILL] * 4]
    h = np.zeros(1024, np.uint32)
    ho = _filled(S, 1, T)
    hp = [P(a) for a in ho]
    for bad in ((8, 1, P(h), 1, 1, 6, 64, T, hp), (S, -1, P(h), 1, 1, 6, 64, T, hp), (S, 1, None, 1, 1, 6, 64, T, hp),
                (S, 1, P(h), 2, 1, 6, 64, T, hp), (S, 1, P(h), 1, -1, 6, 64, T, hp), (S, 1, P(h), 1, 5, 6, 64, T, hp),
                (S, 1, P(h), 1, 1, 0, 64, T, hp), (S, 1, P(h), 1, 1, 33, 64, T, hp), (S, 1, P(h), 1, 1, 6, 0, T, hp),
                (S, 1, P(h), 1, 1, 6, 32769, T, hp), (S, 1, P(h), 1, 1, 6, 64, 65, hp), (S, 1, P(h), 1, 1, 6, 64, T, [None] + hp[1:]),
                (S, 1, P(h), 1, 1, 6, 64, T, hp[:3] + [None, hp[4]]), (S, 1, P(h), 1, 1, 6, 64, T, hp[:4] + [None])):
        s, n, rec, rules, cl, mr, mn, mp, outs = bad
        assert lib.sgo_connect(s, n, rec, None, None, rules, cl, mr, mn, mp, *outs) == SGO_ERR_ARG, bad[:8]
    assert lib.sgo_connect(S, 0, P(h), None, None, 1, 1, 6, 64, T, *hp) == 0
    assert all((a == (FILL16 if a.dtype == np.int16 else FILL)).all() for a in ho)


def test_capturable_in_a_graph():
    """the call alone in a captured graph (its three launches in order), replayed twice over re-filled outputs: the eager result"""
    import torch
    L, lib = _lib()
    S = 9
    names, recs, ask, region, has = CC.case_records(S)
    want = CC.enumerated_model(S, 1)
    R = len(recs)
    dev = torch.device("cuda", 0)
    eager = _run(S, recs, pad=1)                                     # first, so that the capture is not the kernels' first launch
    d_rec = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32)).to(dev)
    out = _filled(S, R + 1, T, dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.sgo_connect_dev(S, R, L.ptr(d_rec), R, None, None, None, 1, CC.CUT_LIBS, CC.MAX_REGION, CC.MAX_NODES, T,
                                 *([L.ptr(t) for t in out] + [L.stream_ptr()]))
    assert rc == 0, lib.sgo_last_error()
    for _ in range(2):
        for t in out:
            t.fill_(FILL16 if t.dtype == torch.int16 else FILL)
        g.replay()
        torch.cuda.synchronize()
        _same(_numpy(*out), want, R, "graph replay")
    assert all(np.array_equal(eager[k], _numpy(*out)[k]) for k in KEYS)


def test_rows_behind_the_grid_cap():
    """131 072 rows of a small case set at max_pairs 2: k_connect_read's gridDim.y is capped at 65 535, so the rows behind take the
    second and third trip of its stride loop; every row is compared with the model of its record"""
    import torch
    S = 5
    names, recs, ask, region, has = CC.case_records(S)
    pick = [names.index(n) for n in ("jump_edge_b", "tiger_corner_w", "fill_b", "side3_w", "false_join_b", "one_chain_b", "stones_far_w")]
    n = 131072
    index = np.resize(np.array(pick, np.int32), n)
    want = M.connect(S, recs, index=pick, rules=1, max_nodes=64, max_pairs=2)
    assert not any((r[:, 6] & (M.A_UNKNOWN | M.D_UNKNOWN)).any() for r in want["rows"]) and {len(r) for r in want["rows"]} == {0, 1, 2}
    got = _run(S, recs, index, max_nodes=64, max_pairs=2, pad=0)
    for j in range(len(pick)):
        sel = slice(j, n, len(pick))
        k = len(want["rows"][j])
        assert (got["n_pairs"][sel] == want["n_pairs"][j]).all(), (names[pick[j]], "n_pairs")
        assert (got["rows"][sel, :k] == want["rows"][j][None]).all() and (got["rows"][sel, k:] == FILL).all(), (names[pick[j]], "rows")
        assert (got["regions"][sel, :k] == want["regions"][j][None]).all(), (names[pick[j]], "regions")
        assert (got["groups"][sel] == want["groups"][j][None]).all() and (got["counts"][sel] == want["counts"][j][None]).all(), (names[pick[j]], "map")


def test_python_surface():
    """connect.connect on host records through an index list, asked and enumerated, and the Connect readers on the named cases"""
    from sejonggo_amd.connect import connect
    S = 7
    names, recs, ask, region, has = CC.case_records(S)
    d, j, c = names.index("diagonal_b"), names.index("jump_b"), names.index("chain3_w")
    v = connect(S, recs, index=[d, -1, j], ask=[ask[d], (0, 1), ask[j]])
    assert len(v) == 3 and v.n_pairs.tolist() == [1, 0, 1]
    p = v.pairs_of(0)[0]
    assert (p.anchor_x, p.anchor_y, p.colour, p.verdict, p.region_empty, p.nodes_a) == (8, 16, 1, "connected", 6, 145)
    assert v.groups_of(0) == {8: [8, 16]} and (v.groups[1] == -1).all() and v.pairs_of(1) == []
    p = v.find(2, 15, 17)
    assert (p.verdict, p.cut_move, p.join_move, p.nodes_a, p.nodes_d) == ("unsettled", 16, 9, 8, 10) and v.groups_of(2) == {15: [15], 17: [17]}
    assert sorted(v.region(2, 0)) == [9, 16, 23]
    v = connect(S, recs, index=[c])
    assert v.verdicts(0) == ["connected", "connected"] and v.group_counts[0].tolist() == [3, 1, 2, 0] and v.groups_of(0) == {8: [8, 16, 24]}
    k = names.index("negative_w")
    v = connect(S, recs, index=[names.index("stones_far_b"), k], ask=[ask[names.index("stones_far_b")], ask[k]])
    assert [(p.open, p.no_pair, p.verdict) for p in (v.pairs_of(0)[0], v.pairs_of(1)[0])] == [(True, False, "open"), (False, True, "no pair")]
