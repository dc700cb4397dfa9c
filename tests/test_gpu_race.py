"""GPU: the capturing-race kernels (include/sgo.h "capturing races", csrc/sgo_race.hip) against the model (tests/race_model.py) word
for word -- n_pairs, table rows and region sets -- at every board size, for both rule sets, asked and enumerated, on the case set
tests/test_race_model_power.py shows to notice the model's fault switches (tests/race_cases.py)."""
import numpy as np
import pytest

from tests import race_cases as RC
from tests import race_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG = -1
FILL = 0x3C3C3C3C
T = 6                                                                # table rows per position in most calls: no case lists more than 4


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _filled(S, n, max_pairs, dev=None):
    """sentinel-filled outputs for n rows: numpy without a device, torch tensors on it"""
    NW = (S * S + 31) // 32
    if dev is None:
        return np.full(n, FILL, np.int32), np.full((n, max_pairs, 16), FILL, np.int32), np.full((n, max_pairs, NW), FILL, np.uint32)
    import torch
    return (torch.full((n,), FILL, dtype=torch.int32, device=dev), torch.full((n, max_pairs, 16), FILL, dtype=torch.int32, device=dev),
            torch.full((n, max_pairs, NW), FILL, dtype=torch.int32, device=dev))


def _numpy(n_pairs, rows, regions):
    return {"n_pairs": n_pairs.cpu().numpy(), "rows": rows.cpu().numpy(), "regions": regions.cpu().numpy().view(np.uint32)}


def _run(S, records, index=None, ask=None, region=None, rules=1, max_libs=RC.MAX_LIBS, max_region=RC.MAX_REGION, max_nodes=RC.MAX_NODES,
         max_pairs=T, n=None, n_records=None, pad=2):
    """sgo_race_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    n = (len(index) if index is not None else len(records)) if n is None else n
    up = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t).view(np.int32)).to(dev)   # noqa: E731
    d_rec, d_idx, d_ask, d_reg = up(records, np.uint32), up(index, np.int32), up(ask, np.int32), up(region, np.uint32)
    out = _filled(S, n + pad, max_pairs, dev)
    rc = lib.sgo_race_dev(S, n, L.ptr(d_rec), len(records) if n_records is None else n_records, L.ptr(d_idx), L.ptr(d_ask), L.ptr(d_reg),
                          rules, max_libs, max_region, max_nodes, max_pairs, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return _numpy(*out)


def _same(got, want, n, what):
    """n_pairs, and every word of the listed rows and region sets; everything behind them is as it was filled"""
    assert got["n_pairs"][:n].tolist() == want["n_pairs"][:n].tolist(), (what, "n_pairs", got["n_pairs"][:n].tolist(), want["n_pairs"][:n].tolist())
    for i in range(n):
        k = len(want["rows"][i])
        assert got["rows"][i, :k].tolist() == want["rows"][i].tolist(), (what, "row", i, got["rows"][i, :k].tolist(), want["rows"][i].tolist())
        assert got["regions"][i, :k].tolist() == want["regions"][i].tolist(), (what, "region", i)
        assert (got["rows"][i, k:] == FILL).all() and (got["regions"][i, k:] == FILL).all(), (what, "rows behind the listed ones", i)
    assert (got["n_pairs"][n:] == FILL).all() and (got["rows"][n:] == FILL).all() and (got["regions"][n:] == FILL).all(), (what, "rows behind n")


def _indexed(want, index, R):
    """the model's outputs of records 0 .. R - 1 re-listed through an index (out of range: no pairs)"""
    NW = want["regions"][0].shape[1]
    ok = [0 <= r < R for r in index]
    return {"n_pairs": np.array([want["n_pairs"][r] if o else 0 for r, o in zip(index, ok)], np.int32),
            "rows": [want["rows"][r] if o else np.zeros((0, 16), np.int32) for r, o in zip(index, ok)],
            "regions": [want["regions"][r] if o else np.zeros((0, NW), np.uint32) for r, o in zip(index, ok)]}


@pytest.mark.parametrize("S", M.SIZES)
def test_case_set_word_for_word(S):
    """every constructed position for both sides to move and both rule sets: asked in the default region and enumerated, in order
    without an index list and with an odd number of rows (the last wave's second half idles in k_race_pairs), and through a list that
    permutes them, repeats some and holds entries out of range; asked in the given regions; the host twin"""
    L, lib = _lib()
    names, recs, ask, region, has = RC.case_records(S)
    R = len(recs)
    rng = np.random.RandomState(S)
    index = np.concatenate([rng.permutation(R), [-1, R, 0, 0, 2 ** 31 - 1, -2 ** 31, R - 1]]).astype(np.int64)
    assert len(index) % 2 == 1
    safe = np.clip(index, 0, R - 1)
    for rules in (1, 0):
        want = RC.asked_model(S, rules)
        _same(_run(S, recs, ask=ask, rules=rules), want, R, ("asked", rules))
        _same(_run(S, recs[:R - 1], ask=ask[:R - 1], rules=rules), want, R - 1, ("asked, odd n", rules))
        _same(_run(S, recs, index.astype(np.int32), ask=ask[safe], rules=rules), _indexed(want, index, R), len(index), ("asked, indexed", rules))
        want = RC.enumerated_model(S, rules)
        _same(_run(S, recs, rules=rules), want, R, ("enumerated", rules))
        _same(_run(S, recs, index.astype(np.int32), ask=np.full((len(index), 2), -1), rules=rules), _indexed(want, index, R), len(index),
              ("enumerated through ask = -1, indexed", rules))
        pick, want = RC.region_model(S, rules)
        _same(_run(S, recs, pick.astype(np.int32), ask=ask[pick], region=region[pick], rules=rules), want, len(pick), ("given regions", rules))
        nt, rows, regs = _filled(S, R, T)
        assert lib.sgo_race(S, R, L.ptr(np.ascontiguousarray(recs)), L.ptr(np.ascontiguousarray(ask)), None, rules, RC.MAX_LIBS, RC.MAX_REGION,
                            RC.MAX_NODES, T, L.ptr(nt), L.ptr(rows), L.ptr(regs)) == 0
        _same({"n_pairs": nt, "rows": rows, "regions": regs}, RC.asked_model(S, rules), R, ("host twin", rules))


def test_max_pairs_cuts_the_table_not_the_count():
    """max_pairs = 1 on positions that list up to four pairs: n_pairs stays, one row is written, the rows behind it are untouched"""
    S = 7
    names, recs, ask, region, has = RC.case_records(S)
    want = RC.enumerated_model(S, 1, max_pairs=1)
    assert max(want["n_pairs"]) >= 3
    _same(_run(S, recs, max_pairs=1), want, len(recs), "max_pairs 1")


def test_node_budget_exact_and_one_less():
    """max_nodes equal to the node count of a query decides it; one less ends it unknown with the count at that moment"""
    S = 7
    names, recs, ask, region, has = RC.case_records(S)
    k = names.index("run_b")
    full = RC.asked_model(S, 1)["rows"][k][0]
    nodes = int(full[12])
    assert nodes > 100 and not full[6] & (M.A_UNKNOWN | M.D_UNKNOWN)
    for budget in (nodes, nodes - 1):
        want = M.race(S, recs[k:k + 1], ask=ask[k:k + 1], rules=1, max_libs=RC.MAX_LIBS, max_region=RC.MAX_REGION, max_nodes=budget)
        assert bool(want["rows"][0][0][6] & M.A_UNKNOWN) == (budget < nodes) and want["rows"][0][0][12] == nodes
        _same(_run(S, recs[k:k + 1], ask=ask[k:k + 1], max_nodes=budget), want, 1, ("budget", budget))


def test_depth_cap():
    """a query whose first line of play passes depth 80 ends unknown there, after 92 nodes; the other racer spends its budget"""
    rec, pq, region = RC.deep_case()
    want = RC.deep_model()
    row = want["rows"][0][0]
    assert row[6] & M.A_UNKNOWN and row[12] == 92 and want["depths"][0][0, 0] == 80
    _same(_run(19, rec[None], ask=[pq], region=region[None], max_libs=RC.DEEP_LIBS, max_region=RC.DEEP_REGION, max_nodes=RC.DEEP_NODES), want, 1,
          "depth cap")


def test_golden_sample_enumerated():
    """plies of the golden play-outs (and, at 19x19, one position of the golden game records) enumerated at (max_libs 4, max_region 5,
    max_nodes 128); each of the four verdicts occurs, so an all-`unknown` reader cannot pass by agreeing with an all-`unknown` model"""
    seen = set()
    for S in M.SIZES:
        recs = RC.golden_sample(S)
        want = RC.golden_model(S)
        got = _run(S, recs, max_libs=RC.GOLDEN_LIBS, max_region=RC.GOLDEN_REGION, max_nodes=RC.GOLDEN_NODES, max_pairs=RC.GOLDEN_PAIRS)
        _same(got, want, len(recs), ("golden", S))
        for i in range(len(recs)):
            for row in got["rows"][i, :min(int(got["n_pairs"][i]), RC.GOLDEN_PAIRS)]:
                seen.update(M.verdicts(row))
    assert seen == {"safe", "unsettled", "caught", "unknown"}, seen


def test_row_counts_and_bad_arguments():
    """n of 0, 1, 2, 3; n_records bounds the index; the refusals leave the outputs as they were"""
    import torch
    L, lib = _lib()
    S = 7
    names, recs, ask, region, has = RC.case_records(S)
    want = RC.asked_model(S, 1)
    idx = np.array([names.index("tiny_b"), names.index("seki_w"), names.index("eye_b")], np.int32)
    for n in (0, 1, 2, 3):
        _same(_run(S, recs, idx[:max(n, 1)], ask=ask[idx[:max(n, 1)]], n=n), _indexed(want, idx[:n], len(recs)), n, n)
    k = int(idx[0])
    _same(_run(S, recs, np.array([k, k + 1], np.int32), ask=ask[[k, k + 1]], n_records=k + 1), _indexed(want, [k, -1], len(recs)), 2, "n_records")
    dev = torch.device("cuda", 0)
    d = torch.zeros(1024, dtype=torch.int32, device=dev)
    nt, rows, regs = _filled(S, 2, T, dev)
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), kw.get("R", 1), None, None, None, kw.get("rules", 1),   # noqa: E731
                         kw.get("libs", 4), kw.get("region", 6), kw.get("nodes", 64), kw.get("pairs", T), kw.get("nt", P(nt)),
                         kw.get("rows", P(rows)), kw.get("regs", P(regs)), L.stream_ptr()]
    for bad in (dict(S=8), dict(S=0), dict(n=-1), dict(R=-1), dict(rules=2), dict(rules=-1), dict(libs=0), dict(libs=9), dict(region=0),
                dict(region=33), dict(nodes=0), dict(nodes=32769), dict(pairs=0), dict(pairs=65), dict(rec=None), dict(nt=None), dict(rows=None),
                dict(regs=None)):
        assert lib.sgo_race_dev(*args(**bad)) == SGO_ERR_ARG, bad
    torch.cuda.synchronize()
    assert (nt == FILL).all() and (rows == FILL).all() and (regs == FILL).all()
    for good in (dict(), dict(libs=1), dict(libs=8), dict(region=1), dict(region=32), dict(nodes=1), dict(nodes=32768), dict(pairs=1)):
        assert lib.sgo_race_dev(*args(**good)) == 0, good              # the empty board: nothing to list
    torch.cuda.synchronize()
    assert nt.tolist() == [0, FILL] and (rows == FILL).all() and (regs == FILL).all()
    h = np.zeros(1024, np.uint32)
    hn, hr, hg = _filled(S, 1, T)
    for bad in ((8, 1, P(h), 1, 4, 6, 64, T, P(hn)), (S, -1, P(h), 1, 4, 6, 64, T, P(hn)), (S, 1, None, 1, 4, 6, 64, T, P(hn)),
                (S, 1, P(h), 2, 4, 6, 64, T, P(hn)), (S, 1, P(h), 1, 0, 6, 64, T, P(hn)), (S, 1, P(h), 1, 9, 6, 64, T, P(hn)),
                (S, 1, P(h), 1, 4, 0, 64, T, P(hn)), (S, 1, P(h), 1, 4, 33, 64, T, P(hn)), (S, 1, P(h), 1, 4, 6, 0, T, P(hn)),
                (S, 1, P(h), 1, 4, 6, 32769, T, P(hn)), (S, 1, P(h), 1, 4, 6, 64, 65, P(hn)), (S, 1, P(h), 1, 4, 6, 64, T, None)):
        s, n, rec, rules, ml, mr, mn, mp, pn = bad
        assert lib.sgo_race(s, n, rec, None, None, rules, ml, mr, mn, mp, pn, P(hr), P(hg)) == SGO_ERR_ARG, bad
    assert lib.sgo_race(S, 0, P(h), None, None, 1, 4, 6, 64, T, P(hn), P(hr), P(hg)) == 0
    assert (hn == FILL).all() and (hr == FILL).all() and (hg == FILL).all()


def test_capturable_in_a_graph():
    """the call alone in a captured graph (its two launches in order), replayed twice over re-filled outputs: the eager result"""
    import torch
    L, lib = _lib()
    S = 9
    names, recs, ask, region, has = RC.case_records(S)
    want = RC.asked_model(S, 1)
    R = len(recs)
    dev = torch.device("cuda", 0)
    eager = _run(S, recs, ask=ask, pad=1)                            # first, so that the capture is not the kernels' first launch
    d_rec = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32)).to(dev)
    d_ask = torch.from_numpy(np.ascontiguousarray(ask)).to(dev)
    out = _filled(S, R + 1, T, dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.sgo_race_dev(S, R, L.ptr(d_rec), R, None, L.ptr(d_ask), None, 1, RC.MAX_LIBS, RC.MAX_REGION, RC.MAX_NODES, T, L.ptr(out[0]),
                              L.ptr(out[1]), L.ptr(out[2]), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    for _ in range(2):
        for t in out:
            t.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        _same(_numpy(*out), want, R, "graph replay")
    assert all(np.array_equal(eager[k], _numpy(*out)[k]) for k in ("n_pairs", "rows", "regions"))


def test_python_surface():
    """race.race on host records through an index list, asked and enumerated, and the Race readers on the named cases"""
    from sejonggo_amd.race import race
    S = 7
    names, recs, ask, region, has = RC.case_records(S)
    t, s, e = names.index("tiny_b"), names.index("seki_b"), names.index("eye_w")
    v = race(S, recs, index=[t, -1, s, e], ask=[ask[t], (0, 1), ask[s], ask[e]], max_libs=RC.MAX_LIBS)
    assert len(v) == 4 and v.n_pairs.tolist() == [1, 0, 1, 1]
    p = v.pairs_of(0)[0]
    assert (p.anchor_b, p.anchor_w, p.black, p.white, p.outcome, p.catch_b) == (1, 2, "caught", "safe", "white wins", 0)
    assert v.region(0, 0) == [0, 3, 4, 10, 11] and v.pairs_of(1) == []
    assert v.pairs_of(2)[0].outcome == "standoff" and v.pairs_of(3)[0].outcome == "black wins" and v.find(3, 1, 4).nodes_ab == 5
    v = race(S, recs, index=[names.index("open_b"), names.index("negative_w")], ask=[ask[names.index("open_b")], ask[names.index("negative_w")]])
    assert [(p.open, p.no_pair, p.outcome, p.black) for p in (v.pairs_of(0)[0], v.pairs_of(1)[0])] == [(True, False, "open", None), (False, True, "no pair", None)]
    v = race(S, recs, index=[t], max_libs=RC.MAX_LIBS)
    assert [(p.anchor_b, p.anchor_w) for p in v.pairs_of(0)] == [tuple(r[:2]) for r in RC.enumerated_model(S, 1)["rows"][t].tolist()]
