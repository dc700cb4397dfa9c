"""GPU: the shape-search kernel (include/sgo.h "shape search", csrc/sgo_shapes.hip) against the model (tests/shapes_model.py) word
for word at every board size, on the case set tests/test_shapes_model_power.py shows to notice the model's fault switches
(tests/shapes_cases.py): every shape -- the windows 1x1, Sx1, 1xS and SxS among them -- over every record."""
import numpy as np
import pytest

from tests import shapes_cases as SC
from tests import shapes_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG = -1
FILL = 0x3C3C3C3C
# chosen on the CPU with the model: each hits some of the twelve golden records of every size and misses some
GOLDEN_SHAPES = ("hook", "side", "row_full", "board_full")


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _table(S, sh):
    """sgo_shape_compile's table of a model Shape, as the library writes it"""
    L, lib = _lib()
    table = np.zeros(M.TABLE_WORDS, np.uint32)
    words = M.struct_words(sh)
    assert lib.sgo_shape_compile(S, L.ptr(words), L.ptr(table)) == 0, lib.sgo_last_error()
    return table


def _run(S, records, index, sh, n=None, n_records=None, pad=2):
    """sgo_shapes_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    NW = (S * S + 31) // 32
    n = (len(index) if index is not None else len(records)) if n is None else n
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev) if index is not None else None
    d_tab = torch.from_numpy(_table(S, sh).view(np.int32)).to(dev)
    hits = torch.full((n + pad, 4), FILL, dtype=torch.int32, device=dev)
    cover = torch.full((n + pad, NW), FILL, dtype=torch.int32, device=dev)
    rc = lib.sgo_shapes_dev(S, n, L.ptr(d_rec), len(records) if n_records is None else n_records, L.ptr(d_idx), L.ptr(d_tab), L.ptr(hits),
                            L.ptr(cover), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return {"hits": hits.cpu().numpy(), "cover": cover.cpu().numpy().view(np.uint32)}


def _same(got, want, n, what):
    """every word of the hits and the cover of rows 0 .. n - 1; the rows behind n are as they were filled"""
    bad = np.flatnonzero((got["hits"][:n] != want["hits"][:n]).any(axis=1))
    assert len(bad) == 0, (what, "hits", bad[:8], got["hits"][bad[:2]], want["hits"][bad[:2]])
    bad = np.flatnonzero((got["cover"][:n] != want["cover"][:n]).any(axis=1))
    assert len(bad) == 0, (what, "cover", bad[:8])
    assert (got["hits"][n:] == FILL).all() and (got["cover"][n:] == FILL).all(), what


def _indexed(want, index, Rn):
    """the model's outputs of records 0 .. Rn - 1 re-listed through an index (out of range: {0, -1, 0, 0} and a zero cover)"""
    out = {"hits": np.zeros((len(index), 4), np.int32), "cover": np.zeros((len(index),) + want["cover"].shape[1:], np.uint32)}
    out["hits"][:, 1] = -1
    for i, r in enumerate(index):
        if 0 <= r < Rn:
            out["hits"][i], out["cover"][i] = want["hits"][r], want["cover"][r]
    return out


@pytest.mark.parametrize("S", M.SIZES)
def test_case_set_word_for_word(S):
    """every shape over every constructed position (both flag values): in order without an index list, through a list that
    permutes the records, repeats some and holds entries out of range, and through the host twin"""
    L, lib = _lib()
    names, recs = SC.case_records(S)
    Rn, NW = len(recs), (S * S + 31) // 32
    rng = np.random.RandomState(S)
    index = np.concatenate([rng.permutation(Rn), [-1, Rn, 0, 0, 2 ** 31 - 1, -2 ** 31, Rn - 1, 1, Rn + 7]]).astype(np.int64)
    for name, sh in SC.shapes(S).items():
        want = SC.case_model(S, name)
        _same(_run(S, recs, None, sh), want, Rn, (name, "in order"))
        _same(_run(S, recs, index.astype(np.int32), sh), _indexed(want, index, Rn), len(index), (name, "indexed"))
        hits, cover = np.full((Rn + 1, 4), FILL, np.int32), np.full((Rn + 1, NW), FILL, np.uint32)
        words = M.struct_words(sh)
        assert lib.sgo_shapes(S, Rn, L.ptr(np.ascontiguousarray(recs)), L.ptr(words), L.ptr(hits), L.ptr(cover)) == 0
        _same({"hits": hits, "cover": cover}, want, Rn, (name, "host twin"))


@pytest.mark.parametrize("S", M.SIZES)
def test_golden_positions(S):
    """positions the reference's random games reached (the records tests/keys_model.py draws): each chosen shape hits some and
    misses some, so the comparison is about both"""
    from tests.keys_model import golden_records
    recs = golden_records(S)
    for name in GOLDEN_SHAPES:
        sh = SC.shapes(S)[name]
        want = M.shapes(S, recs, sh)
        hit = want["hits"][:, 0] > 0
        assert hit.any() and not hit.all(), name
        _same(_run(S, recs, None, sh), want, len(recs), ("golden", name))


def test_windows_across_the_lane_boundaries_at_19():
    """S = 19: three-row windows that start in rows 14, 15 and 16 (lanes 15 | 16 are two DPP rows); a 19-row window whose cells are
    don't-care but for the last, in the half beside a record with a full first row (nothing of the neighbour may leak in); a window
    in the last column and in the last row"""
    S = 19
    names, recs = SC.case_records(S)
    sh = SC.shapes(S)
    k = names.index("rows3_b")
    black, white, _ = M.record_stones(S, recs[k])
    _, _, matches = M.point_shapes(S, black, white, sh["rows3"])
    assert {14, 15, 16} <= {y0 for v, x0, y0 in matches if v == 0}
    _same(_run(S, recs, [k], sh["rows3"]), _indexed(SC.case_model(S, "rows3"), [k], len(recs)), 1, "rows3")
    # pairs of records that share a wavefront: (even row, odd row)
    pick = [names.index(n) for n in ("empty_b", "top_row_b", "bottom_row_b", "top_row_w", "top_row_b", "empty_w", "col_full_b", "top_row_b",
                                     "last_point_b", "bottom_row_b", "top_row_w")]
    for shape in ("col_full", "stone_dc", "stone_e", "board_full", "gap"):
        want = _indexed(SC.case_model(S, shape), pick, len(recs))
        if shape == "col_full":
            assert want["hits"][0].tolist() == [0, -1, 0, 0] and want["hits"][2, 0] > 0 and want["hits"][6, 0] > 0
        _same(_run(S, recs, pick, sh[shape]), want, len(pick), shape)


def test_flag_beside_an_empty_last_point_at_5():
    """S = 5: the to-play flag shares the only word with the stones; point 24 is empty and is found empty, the flag is no stone"""
    S = 5
    names, recs = SC.case_records(S)
    k = names.index("flag_corner_w")
    assert recs[k][0] >> 31 == 1 and not (recs[k][0] >> 24) & 1 and not (recs[k][1] >> 24) & 1
    for shape in ("gap", "stone", "stone_e"):
        want = _indexed(SC.case_model(S, shape), [k], len(recs))
        if shape == "gap":
            assert (want["cover"][0, 0] >> 24) & 1 and want["cover"][0, 0] >> 25 == 0 and want["hits"][0, 0] == 22
        _same(_run(S, recs, [k], SC.shapes(S)[shape]), want, 1, shape)


def test_row_counts_and_bad_arguments():
    """n of 0, 1, 2, 3 (odd: a half without a record); n_records bounds the index; the refusals"""
    import torch
    L, lib = _lib()
    S = 9
    names, recs = SC.case_records(S)
    sh = SC.shapes(S)["hook"]
    want = SC.case_model(S, "hook")
    idx = (np.arange(7) * 5 % len(recs) + names.index("hook@1,1_b")).astype(np.int32) % len(recs)
    assert want["hits"][idx[0], 0] > 0
    for n in (0, 1, 2, 3, 7):
        _same(_run(S, recs, idx[:max(n, 1)], sh, n=n), _indexed(want, idx[:n], len(recs)), n, n)
    _same(_run(S, recs[:3], None, sh, n=3), {"hits": want["hits"][:3], "cover": want["cover"][:3]}, 3, "no index, odd n")
    k = names.index("hook@1,1_b")
    got = _run(S, recs, np.array([k, k + 1], np.int32), sh, n_records=k + 1)
    _same(got, _indexed(want, [k, -1], len(recs)), 2, "n_records")
    dev = torch.device("cuda", 0)
    d, d1, d2 = (torch.zeros(1024, dtype=torch.int32, device=dev) for _ in range(3))
    tab = torch.from_numpy(_table(S, sh).view(np.int32)).to(dev)
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), kw.get("nr", 1), None, kw.get("tab", P(tab)),   # noqa: E731
                         kw.get("hits", P(d1)), kw.get("cover", P(d2)), L.stream_ptr()]
    assert lib.sgo_shapes_dev(*args()) == 0
    for bad in (dict(S=8), dict(S=0), dict(n=-1), dict(nr=-1), dict(rec=None), dict(tab=None), dict(hits=None), dict(cover=None)):
        assert lib.sgo_shapes_dev(*args(**bad)) == SGO_ERR_ARG, bad
    h, h1, h2 = (np.zeros(1024, np.uint32) for _ in range(3))
    words = M.struct_words(sh)
    assert lib.sgo_shapes(8, 1, P(h), P(words), P(h1), P(h2)) == SGO_ERR_ARG
    assert lib.sgo_shapes(S, -1, P(h), P(words), P(h1), P(h2)) == SGO_ERR_ARG
    assert lib.sgo_shapes(S, 1, None, P(words), P(h1), P(h2)) == SGO_ERR_ARG
    assert lib.sgo_shapes(S, 1, P(h), None, P(h1), P(h2)) == SGO_ERR_ARG
    assert lib.sgo_shapes(S, 1, P(h), P(words), None, P(h2)) == SGO_ERR_ARG
    assert lib.sgo_shapes(S, 1, P(h), P(words), P(h1), None) == SGO_ERR_ARG
    wide = words.copy()
    wide[0] = S + 1
    assert lib.sgo_shapes(S, 1, P(h), P(wide), P(h1), P(h2)) == SGO_ERR_ARG            # a shape the compiler refuses
    assert lib.sgo_shapes(S, 0, P(h), P(words), P(h1), P(h2)) == 0
    torch.cuda.synchronize()


def test_python_surface_and_record_set():
    """shapes.shapes on host records, and RecordSet.find over the golden 19x19 collection in one chunk: the first matching ply of
    every game is the model's"""
    from sejonggo_amd.records import Record, RecordSet
    from sejonggo_amd.shapes import Shape, shapes
    from tests.fake_shapes_records import model_shape
    from tests.helpers import load
    from tests.tactics_cases import golden_records
    S = 5
    names, recs = SC.case_records(S)
    k = names.index("hook@1,1_b")
    hook = Shape.parse(".XO/*X.")
    v = shapes(S, recs, hook, index=[k, -1])
    assert v.hits[0].tolist() == SC.case_model(S, "hook")["hits"][k].tolist() and v.first(0) == (0, 1, 1) and v.first(1) is None
    assert v.cover(0) == [6, 7, 8, 12, 13] and v.cover(1) == [] and v.hits[1].tolist() == [0, -1, 0, 0]
    z = load("sgf_S19.npz")
    games = []
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        entries = [(19 * 19 if y >= 19 else int(y) * 19 + int(x), int(c)) for x, y, c in mv]
        games.append(Record("g%d" % gi, 19, entries, [False] * len(entries), list(range(1, len(entries) + 1)), None))
    # a lone stone on the 3-4 point of an empty corner, in either colour and any orientation: the opening of some of the games
    corner = Shape.parse("+-----\n|.....\n|.....\n|...X.\n|.....\n|.....")
    rs = RecordSet(games, size=19)
    try:
        chunks = list(rs.shapes(corner))
        assert len(chunks) == 1
        gold = M.shapes(19, golden_records(), model_shape(corner))
        assert np.array_equal(chunks[0].shapes.hits[::4], gold["hits"]) and np.array_equal(chunks[0].shapes.cover_words[::4], gold["cover"])
        assert (gold["hits"][:, 0] > 0).sum() == 7
        found = rs.find(corner)
        assert found["searched"] == 5 and found["matched"] == len(found["games"]) >= 2
        base = 0
        by = {d["name"]: d for d in found["games"]}
        for g in games:
            rows = np.flatnonzero(chunks[0].shapes.hits[base:base + len(g.entries) + 1, 0] > 0)
            assert (g.name in by) == bool(len(rows))
            if len(rows):
                assert by[g.name]["ply"] == int(rows[0])
            base += len(g.entries) + 1
        assert sum(d["count"] for d in found["continuations"]) == found["matched"]
    finally:
        rs.close()
