"""GPU: the unconditional-life kernel (include/sgo.h "unconditional life", csrc/sgo_life.hip) against the model
(tests/life_model.py) word for word at every board size, on the case set tests/test_life_model_power.py shows to notice the model's
fault switches (tests/life_cases.py)."""
import numpy as np
import pytest

from tests import life_cases as LC
from tests import life_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG = -1
FILL = 0x3C3C3C3C


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _run(S, records, index, n=None, n_records=None, pad=2):
    """sgo_life_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    NW = (S * S + 31) // 32
    n = (len(index) if index is not None else len(records)) if n is None else n
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev) if index is not None else None
    sets = torch.full((n + pad, 4, NW), FILL, dtype=torch.int32, device=dev)
    counts = torch.full((n + pad, 8), FILL, dtype=torch.int32, device=dev)
    rc = lib.sgo_life_dev(S, n, L.ptr(d_rec), len(records) if n_records is None else n_records, L.ptr(d_idx), L.ptr(sets), L.ptr(counts),
                          L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return {"sets": sets.cpu().numpy().view(np.uint32), "counts": counts.cpu().numpy()}


def _same(got, want, n, what):
    """every word of the sets and the counts of rows 0 .. n - 1; the rows behind n are as they were filled"""
    bad = np.flatnonzero((got["counts"][:n] != want["counts"][:n]).any(axis=1))
    assert len(bad) == 0, (what, "counts", bad[:8], got["counts"][bad[:2]], want["counts"][bad[:2]])
    bad = np.flatnonzero((got["sets"][:n] != want["sets"][:n]).any(axis=(1, 2)))
    assert len(bad) == 0, (what, "sets", bad[:8])
    assert (got["sets"][n:] == FILL).all() and (got["counts"][n:] == FILL).all(), what


def _indexed(want, index, R):
    """the model's outputs of records 0 .. R - 1 re-listed through an index (out of range: the zero row)"""
    out = {"sets": np.zeros((len(index),) + want["sets"].shape[1:], np.uint32), "counts": np.zeros((len(index), 8), np.int32)}
    for i, r in enumerate(index):
        if 0 <= r < R:
            out["sets"][i], out["counts"][i] = want["sets"][r], want["counts"][r]
    return out


@pytest.mark.parametrize("S", M.SIZES)
def test_case_set_word_for_word(S):
    """every constructed position (both flag values, both colour assignments) and the rule shapes: in order without an index list,
    then through a list that permutes them, repeats some and holds entries out of range; the host twin"""
    L, lib = _lib()
    names, recs = LC.case_records(S)
    want = LC.case_model(S)
    R = len(recs)
    _same(_run(S, recs, None), want, R, "in order")
    rng = np.random.RandomState(S)
    index = np.concatenate([rng.permutation(R), [-1, R, 0, 0, 2 ** 31 - 1, -2 ** 31, R - 1, 1, R + 7]]).astype(np.int64)
    _same(_run(S, recs, index.astype(np.int32)), _indexed(want, index, R), len(index), "indexed")
    NW = (S * S + 31) // 32
    sets, counts = np.full((R + 1, 4, NW), FILL, np.uint32), np.full((R + 1, 8), FILL, np.int32)
    assert lib.sgo_life(S, R, L.ptr(np.ascontiguousarray(recs)), L.ptr(sets), L.ptr(counts)) == 0
    _same({"sets": sets, "counts": counts}, want, R, "host twin")


def test_golden_positions():
    """every fourth position of the five golden 19x19 games (the records model replays them): one call"""
    recs = LC.golden_records()
    _same(_run(19, recs, None), LC.golden_model(), len(recs), "golden")


def test_the_long_cascade_beside_short_rows():
    """the 19x19 open diagonal (19 passes for one colour, one for the other) between rows that end at once: the halves of its
    wavefront finish far apart, and so do neighbouring workgroups"""
    S = 19
    names, recs = LC.case_records(S)
    want = LC.case_model(S)
    pick = np.array([names.index(k) for k in ("empty_sb", "cascade_sb", "cascade_cw", "word_bounds_sw", "cascade_cb", "lattice_sb")], np.int32)
    assert want["rounds"][pick[1]].tolist() == [19, 1] and want["rounds"][pick[2]].tolist() == [1, 19]
    _same(_run(S, recs, pick), _indexed(want, pick, len(recs)), len(pick), "cascade")


def test_row_counts_and_bad_arguments():
    """n of 0, 1, 2, 3; n_records bounds the index; the refusals"""
    import torch
    L, lib = _lib()
    S = 9
    names, recs = LC.case_records(S)
    want = LC.case_model(S)
    idx = (np.arange(7) * 5 % len(recs)).astype(np.int32)
    for n in (0, 1, 2, 3, 7):
        _same(_run(S, recs, idx[:max(n, 1)], n=n), _indexed(want, idx[:n], len(recs)), n, n)
    k = names.index("two_eyes_sb")
    got = _run(S, recs, np.array([k, k + 1], np.int32), n_records=k + 1)
    _same(got, _indexed(want, [k, -1], len(recs)), 2, "n_records")
    dev = torch.device("cuda", 0)
    d, d1, d2 = (torch.zeros(1024, dtype=torch.int32, device=dev) for _ in range(3))
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), kw.get("nr", 1), None, kw.get("sets", P(d1)),   # noqa: E731
                         kw.get("counts", P(d2)), L.stream_ptr()]
    assert lib.sgo_life_dev(*args()) == 0
    for bad in (dict(S=8), dict(S=0), dict(n=-1), dict(nr=-1), dict(rec=None), dict(sets=None), dict(counts=None)):
        assert lib.sgo_life_dev(*args(**bad)) == SGO_ERR_ARG, bad
    h, h1, h2 = (np.zeros(1024, np.uint32) for _ in range(3))
    assert lib.sgo_life(8, 1, P(h), P(h1), P(h2)) == SGO_ERR_ARG
    assert lib.sgo_life(S, -1, P(h), P(h1), P(h2)) == SGO_ERR_ARG
    assert lib.sgo_life(S, 1, None, P(h1), P(h2)) == SGO_ERR_ARG
    assert lib.sgo_life(S, 1, P(h), None, P(h2)) == SGO_ERR_ARG
    assert lib.sgo_life(S, 1, P(h), P(h1), None) == SGO_ERR_ARG
    assert lib.sgo_life(S, 0, P(h), P(h1), P(h2)) == 0
    torch.cuda.synchronize()


def test_python_surface_and_record_set():
    """life.life on host records, and RecordSet.life over the golden collection in one chunk: row ch.index[e] is the position
    before entry e (every fourth is one of the model's golden rows)"""
    from sejonggo_amd.life import format_board, life
    from sejonggo_amd.records import Record, RecordSet, life_lines
    from tests.helpers import load
    S = 5
    names, recs = LC.case_records(S)
    want = LC.case_model(S)
    k = names.index("settled_sw")
    v = life(S, recs, index=[k, -1])
    assert v.counts[0].tolist() == want["counts"][k].tolist() and v.settled(0) and v.margin(0) == 5
    assert v.territory(0, 1) == [0, 10] and v.territory(0, -1) == [4, 14] and not v.counts[1].any() and not v.sets[1].any()
    assert format_board(v, 0).split("\n")[-1] == "settled 25/25 black 15 white 10"
    z = load("sgf_S19.npz")
    games = []
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        entries = [(19 * 19 if y >= 19 else int(y) * 19 + int(x), int(c)) for x, y, c in mv]
        games.append(Record("g%d" % gi, 19, entries, [False] * len(entries), list(range(1, len(entries) + 1)), None))
    rs = RecordSet(games, size=19)
    try:
        chunks = list(rs.life())
        assert len(chunks) == 1
        vv = chunks[0].life
        gold = LC.golden_model()
        assert np.array_equal(vv.counts[::4], gold["counts"]) and np.array_equal(vv.sets[::4], gold["sets"])
        lines = life_lines(rs)
        assert [d["plies"] for d in lines] == [len(g.entries) for g in games]
        base = 0
        for d, g in zip(lines, games):
            rows = vv.counts[base:base + len(g.entries) + 1]
            first = np.flatnonzero(rows[:, :2].sum(axis=1) > 0)
            assert d["first_alive"] == (int(first[0]) if len(first) else None) and d["unsettled"] == int(rows[-1, 6])
            base += len(g.entries) + 1
    finally:
        rs.close()
