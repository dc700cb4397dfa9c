"""GPU: the influence kernel (include/sgo.h "influence", csrc/sgo_influence.hip) against the model (tests/influence_model.py) word
for word -- every value, set word and count -- at every board size and at the five parameter triples, on the case set
tests/test_influence_model_power.py shows to notice the model's fault switches (tests/influence_cases.py).  No call lists more than
64 rows."""
import numpy as np
import pytest

from tests import influence_cases as IC
from tests import influence_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG = -1
FILL, FILL16 = 0x3C3C3C3C, 0x3C3C
KEYS = ("values", "sets", "counts")


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _run(S, records, index, dead, triple, n=None, n_records=None, pad=2):
    """sgo_influence_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    N, NW = S * S, (S * S + 31) // 32
    n = (len(index) if index is not None else len(records)) if n is None else n
    assert n <= 64
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev) if index is not None else None
    d_dead = torch.from_numpy(np.ascontiguousarray(dead, np.uint32).view(np.int32)).to(dev) if dead is not None else None
    values = torch.full((n + pad, N), FILL16, dtype=torch.int16, device=dev)
    sets = torch.full((n + pad, 4, NW), FILL, dtype=torch.int32, device=dev)
    counts = torch.full((n + pad, 8), FILL, dtype=torch.int32, device=dev)
    rc = lib.sgo_influence_dev(S, n, L.ptr(d_rec), len(records) if n_records is None else n_records, L.ptr(d_idx), L.ptr(d_dead),
                               triple[0], triple[1], triple[2], L.ptr(values), L.ptr(sets), L.ptr(counts), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return {"values": values.cpu().numpy(), "sets": sets.cpu().numpy().view(np.uint32), "counts": counts.cpu().numpy()}


def _same(got, want, n, what):
    """every word of the values, the sets and the counts of rows 0 .. n - 1; the rows behind n are as they were filled"""
    for k in KEYS:
        width = int(np.prod(got[k].shape[1:]))
        g, w = got[k][:n].reshape(n, width), want[k][:n].reshape(n, width)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert len(bad) == 0, (what, k, bad[:8], g[bad[:1]], w[bad[:1]])
    assert (got["values"][n:] == FILL16).all() and (got["sets"][n:] == FILL).all() and (got["counts"][n:] == FILL).all(), what


def _indexed(want, index, R):
    """the model's outputs of records 0 .. R - 1 re-listed through an index (out of range: the zero row)"""
    out = {k: np.zeros((len(index),) + want[k].shape[1:], want[k].dtype) for k in KEYS}
    for i, r in enumerate(index):
        if 0 <= r < R:
            for k in KEYS:
                out[k][i] = want[k][r]
    return out


@pytest.mark.parametrize("S", M.SIZES)
def test_case_set_word_for_word(S):
    """every named case (as drawn and colours swapped, both flag values, each with its `dead` row -- zero rows but for dead_inside,
    whose row holds stray bits on empty points and bits >= N) at all five triples; with d_dead NULL; the host twin; positions of
    play (rule shapes, golden positions at 19x19)"""
    L, lib = _lib()
    names, recs, dead = IC.case_records(S)
    R = len(recs)
    for triple in M.TRIPLES:
        _same(_run(S, recs, None, dead, triple), IC.case_model(S, triple), R, ("cases", triple))
    for triple in (M.TERRITORY, (1, 0, 1)):
        want = IC.case_model(S, triple, False)
        _same(_run(S, recs, None, None, triple), want, R, ("no dead", triple))
        N, NW = S * S, (S * S + 31) // 32
        values, sets = np.full((R + 1, N), FILL16, np.int16), np.full((R + 1, 4, NW), FILL, np.uint32)
        counts = np.full((R + 1, 8), FILL, np.int32)
        assert lib.sgo_influence(S, R, L.ptr(np.ascontiguousarray(recs)), None, triple[0], triple[1], triple[2], L.ptr(values), L.ptr(sets),
                                 L.ptr(counts)) == 0
        _same({"values": values, "sets": sets, "counts": counts}, want, R, ("host twin", triple))
    values[:], sets[:], counts[:] = FILL16, FILL, FILL
    assert lib.sgo_influence(S, R, L.ptr(np.ascontiguousarray(recs)), L.ptr(np.ascontiguousarray(dead)), 5, 10, 21, L.ptr(values),
                             L.ptr(sets), L.ptr(counts)) == 0
    _same({"values": values, "sets": sets, "counts": counts}, IC.case_model(S, M.TERRITORY), R, "host twin with dead")
    extra = IC.extra_records(S)
    _same(_run(S, extra, None, None, M.TERRITORY), IC.extra_model(S, M.TERRITORY), len(extra), "play")


@pytest.mark.parametrize("S", M.SIZES)
def test_index_lists_odd_n_and_dead_rows_follow_the_row(S):
    """an index list that permutes the cases, repeats some and holds entries out of range, of odd length; `dead` is per ROW: the
    dead_inside set is given to other records too (where it lifts other stones or nothing)"""
    names, recs, dead = IC.case_records(S)
    R = len(recs)
    rng = np.random.RandomState(S)
    index = np.concatenate([rng.permutation(R), [-1, R, 0, 0, 2 ** 31 - 1, -2 ** 31, R - 1, 1, R + 7]]).astype(np.int64)
    assert len(index) % 2 == 1 and len(index) <= 64
    rows = np.stack([dead[names.index("dead_inside_sb")] if i % 3 == 0 else dead[0] for i in range(len(index))])
    rows[1] = 0xFFFFFFFF                                             # every stone of that row is lifted
    for triple in (M.TERRITORY, (8, 31, 31)):
        want = M.influence(S, recs, index, rows, *triple)
        assert not want["counts"][1].any() or want["counts"][1, 4:6].tolist() == [0, 0]
        _same(_run(S, recs, index.astype(np.int32), rows, triple), want, len(index), ("indexed", triple))
        for n in (0, 1, 2, 3, 7):
            _same(_run(S, recs, index[:max(n, 1)].astype(np.int32), rows[:max(n, 1)], triple, n=n),
                  {k: want[k][:n] for k in KEYS}, n, (n, triple))
    k = names.index("walls_sb")
    got = _run(S, recs, np.array([k, k + 1], np.int32), None, M.TERRITORY, n_records=k + 1)
    _same(got, _indexed(IC.case_model(S, M.TERRITORY, False), [k, -1], R), 2, "n_records")


def _edge_pair(S, first_black):
    """two records for the two halves of one wavefront: a full last row in half 0 beside a full first row of the other colour in
    half 1"""
    from tests.life_model import build_record
    last, first = [(S - 1) * S + x for x in range(S)], list(range(S))
    a = build_record(S, last if first_black else [], [] if first_black else last, False)
    b = build_record(S, [] if first_black else first, first if first_black else [], True)
    return np.stack([a, b])


@pytest.mark.parametrize("S", (19, 5))
def test_nothing_leaks_between_the_halves_of_a_wave(S):
    """a full black last row in the record of half 0 beside a white first row in the record of half 1, and the reverse; then each
    beside an empty board, an out-of-range row and a missing row (odd n).  Stones on the last row and column at every triple."""
    for first_black in (True, False):
        recs = _edge_pair(S, first_black)
        for triple in M.TRIPLES:
            _same(_run(S, recs, None, None, triple), M.influence(S, recs, None, None, *triple), 2, ("pair", first_black, triple))
        for index in ([0, -1, 1, 0], [1, 0, 0], [-1, 1, 5, 0, 1]):
            want = M.influence(S, recs, index, None, *M.TERRITORY)
            _same(_run(S, recs, np.array(index, np.int32), None, M.TERRITORY), want, len(index), ("pair", first_black, index))


def test_refusals():
    import torch
    L, lib = _lib()
    S = 9
    dev = torch.device("cuda", 0)
    d = torch.zeros(1024, dtype=torch.int32, device=dev)
    v = torch.full((2, 81), FILL16, dtype=torch.int16, device=dev)
    s, c = (torch.full((2, 4 * 3 if k == 0 else 8), FILL, dtype=torch.int32, device=dev) for k in range(2))
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), kw.get("nr", 1), None, None, kw.get("dilate", 5),   # noqa: E731
                         kw.get("moyo", 10), kw.get("terr", 21), kw.get("values", P(v)), kw.get("sets", P(s)), kw.get("counts", P(c)),
                         L.stream_ptr()]
    assert lib.sgo_influence_dev(*args()) == 0
    torch.cuda.synchronize()
    assert c[0].tolist() == [0, 0, 0, 0, 0, 0, 81, 0] and (c[1] == FILL).all() and not v[0].any() and (v[1] == FILL16).all()
    for bad in (dict(S=8), dict(S=0), dict(n=-1), dict(nr=-1), dict(rec=None), dict(values=None), dict(sets=None), dict(counts=None),
                dict(dilate=-1), dict(dilate=9), dict(moyo=-1), dict(terr=32), dict(moyo=32, terr=32), dict(moyo=11, terr=10)):
        assert lib.sgo_influence_dev(*args(**bad)) == SGO_ERR_ARG, bad
    assert lib.sgo_influence_dev(*args(dilate=8, moyo=31, terr=31)) == 0 and lib.sgo_influence_dev(*args(dilate=0, moyo=0, terr=0)) == 0
    assert lib.sgo_influence_dev(*args(n=0, values=None)) == SGO_ERR_ARG and lib.sgo_influence_dev(*args(n=0)) == 0
    h = np.zeros(1024, np.uint32)
    hv, hs, hc = np.full((1, 81), FILL16, np.int16), np.full((1, 4, 3), FILL, np.uint32), np.full((1, 8), FILL, np.int32)
    call = lambda S_=S, n=1, rec=P(h), t=(5, 10, 21), values=P(hv), sets=P(hs), counts=P(hc): lib.sgo_influence(   # noqa: E731
        S_, n, rec, None, t[0], t[1], t[2], values, sets, counts)
    assert call(S_=8) == SGO_ERR_ARG and call(n=-1) == SGO_ERR_ARG and call(rec=None) == SGO_ERR_ARG
    assert call(values=None) == SGO_ERR_ARG and call(sets=None) == SGO_ERR_ARG and call(counts=None) == SGO_ERR_ARG
    assert call(t=(9, 0, 0)) == SGO_ERR_ARG and call(t=(5, 11, 10)) == SGO_ERR_ARG and call(t=(5, 0, 32)) == SGO_ERR_ARG
    assert call(n=0) == 0 and (hv == FILL16).all() and (hs == FILL).all() and (hc == FILL).all()
    torch.cuda.synchronize()


def test_capturable_in_a_graph():
    """the call alone in a captured graph, replayed once over re-filled outputs: the eager result"""
    import torch
    L, lib = _lib()
    S = 13
    names, recs, dead = IC.case_records(S)
    want = IC.case_model(S, M.TERRITORY)
    R, N, NW = len(recs), S * S, (S * S + 31) // 32
    dev = torch.device("cuda", 0)
    eager = _run(S, recs, None, dead, M.TERRITORY, pad=1)          # first, so that the capture is not the kernel's first launch
    d_rec = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32)).to(dev)
    d_dead = torch.from_numpy(np.ascontiguousarray(dead).view(np.int32)).to(dev)
    values = torch.full((R + 1, N), FILL16, dtype=torch.int16, device=dev)
    sets = torch.full((R + 1, 4, NW), FILL, dtype=torch.int32, device=dev)
    counts = torch.full((R + 1, 8), FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.sgo_influence_dev(S, R, L.ptr(d_rec), R, None, L.ptr(d_dead), 5, 10, 21, L.ptr(values), L.ptr(sets), L.ptr(counts),
                                   L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    values.fill_(FILL16)
    sets.fill_(FILL)
    counts.fill_(FILL)
    g.replay()
    torch.cuda.synchronize()
    got = {"values": values.cpu().numpy(), "sets": sets.cpu().numpy().view(np.uint32), "counts": counts.cpu().numpy()}
    _same(got, want, R, "graph replay")
    assert all(np.array_equal(eager[k], got[k]) for k in KEYS)


def test_python_surface():
    """influence.influence on host records with an index and a `dead` array"""
    from sejonggo_amd.influence import PRESETS, influence
    S = 5
    names, recs, dead = IC.case_records(S)
    k = names.index("dead_inside_sb")
    v = influence(S, recs, index=[k, -1, k], dead=np.stack([dead[k], dead[k], dead[0]]))
    want = IC.case_model(S, M.TERRITORY)
    assert np.array_equal(v.values[0], want["values"][k]) and np.array_equal(v.sets[0], want["sets"][k])
    assert v.counts[0].tolist() == want["counts"][k].tolist() and not v.counts[1].any() and not v.values[1].any()
    assert v.counts[2].tolist() == IC.case_model(S, M.TERRITORY, False)["counts"][k].tolist()
    a = influence(S, recs, **PRESETS["area"])
    assert np.array_equal(a.counts, IC.case_model(S, M.AREA, False)["counts"])
    with pytest.raises(ValueError):
        influence(S, recs, dead=dead[:3])
    with pytest.raises(ValueError):
        influence(S, recs[:, :-1])
