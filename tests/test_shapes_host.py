"""CPU: the host side of the shape search -- sgo_shape_compile through the loaded library against the model's tables
(tests/shapes_model.py), shapes.Shape.parse and its variants, and records.RecordSet.find, `review --find`, `records --find` and
GTP's `sgo-find` on the fake replay object with the model behind it (tests/fake_shapes_records.py) and on a scripted engine; no
GPU."""
import ctypes as C
import io
import json

import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review
from sejonggo_amd import shapes as shapes_mod
from sejonggo_amd.sgfload import SgfGame
from tests import shapes_cases as SC
from tests import shapes_model as M
from tests.fake_shapes_records import ShapesRecords, model_shape

S = 5
SGO_ERR_ARG = -1
P = lambda x, y: y * S + x                                                               # noqa: E731
HOOK = ".XO/*X."

# the hook appears with black's third stone at (1, 1) as drawn; white then plays on its empty cell (0, 0) and wins
GAME_A = [(P(2, 1), 1), (P(3, 1), -1), (P(2, 2), 1), (P(1, 1), -1), (S * S, 1)]
# the same shape turned (k = 4 of the symmetry tables: (x, y) -> (4 - y, x)) in the other colours; the next move is far away
_T = lambda a: (a % S) * S + (S - 1 - a // S)                                            # noqa: E731
GAME_B = [(_T(P(2, 1)), -1), (_T(P(3, 1)), 1), (_T(P(2, 2)), -1), (P(0, 4), 1)]
GAME_C = [(P(0, 0), 1), (P(4, 4), -1)]                                                   # never
GAME_D = GAME_A[:3]                                                                      # the game ends on the match


def _lib():
    from sejonggo_amd import _lib as L
    from sejonggo_amd.build import build_lib
    build_lib()
    return L, L.load()


def _compile(lib, L, size, words):
    """(rc, table) of sgo_shape_compile on the 61 words of an sgo_shape; the table is pre-filled"""
    table = np.full(M.TABLE_WORDS, 0x5A5A5A5A, np.uint32)
    words = np.ascontiguousarray(words, np.uint32)
    return lib.sgo_shape_compile(size, L.ptr(words), L.ptr(table)), table


@pytest.mark.parametrize("size", M.SIZES)
def test_compile_equals_the_models_table(size):
    """every case shape at every size, word for word: header, kept mask, the slots of the kept variants, zeros elsewhere"""
    L, lib = _lib()
    for name, sh in SC.shapes(size).items():
        rc, table = _compile(lib, L, size, M.struct_words(sh))
        assert rc == 0, (name, lib.sgo_last_error())
        assert np.array_equal(table, M.table(size, sh)), name
    sh = SC.shapes(size)
    for name, mask in (("stone", 0x0101), ("pair", 0x0303), ("stone_dc", 0x4747), ("corner", 0x2D2D), ("rows3", 0x001B), ("hook", 0xFFFF)):
        rc, table = _compile(lib, L, size, M.struct_words(sh[name]))
        assert rc == 0 and int(table[2]) == mask and int(table[1]) == bin(mask).count("1"), name
        assert [int(table[16 + 64 * t]) for t in range(int(table[1]))] == [v for v in range(16) if mask >> v & 1]


def test_compile_through_the_python_struct():
    L, lib = _lib()
    sh = shapes_mod.Shape.parse("+---\n|*X.\n|XO.\n|...")
    assert np.array_equal(np.frombuffer(bytes(sh.to_struct()), np.uint32), M.struct_words(SC.shapes(S)["corner"]))
    assert np.array_equal(shapes_mod.compile_table(9, sh), M.table(9, SC.shapes(9)["corner"]))
    # the pure-Python variants are the table's
    table = shapes_mod.compile_table(9, shapes_mod.Shape.parse(HOOK))
    for t, var in enumerate(shapes_mod.Shape.parse(HOOK).variants()):
        slot = table[16 + 64 * t:16 + 64 * (t + 1)]
        assert [int(a) for a in slot[:4]] == [var.v, var.w, var.h, var.edges]
        want = M.struct_words(M.Shape(var.w, var.h, var.edges, var.cells))
        assert np.array_equal(slot[4:61], want[4:])


def test_compile_refusals():
    L, lib = _lib()
    good = M.struct_words(M.shape(["X.", "O*"], M.L))

    def refused(size=S, **change):
        w = good.copy()
        for k, v in change.items():
            w[int(k[1:])] = np.uint32(v & 0xFFFFFFFF)
        rc, table = _compile(lib, L, size, w)
        assert (table == 0x5A5A5A5A).all() or rc == 0              # a refusal writes nothing
        return rc == SGO_ERR_ARG

    assert _compile(lib, L, S, good)[0] == 0
    assert refused(size=8) and refused(size=0)                      # an unsupported size
    assert refused(w0=0) and refused(w0=S + 1) and refused(w0=-1)   # w outside [1, S]
    assert refused(w1=0) and refused(w1=S + 1)                      # h
    assert not refused(size=19, w0=19, w1=19) and refused(size=19, w0=20)
    assert refused(w2=16) and refused(w2=-1)                        # edges outside [0, 15]
    assert refused(w3=1)                                            # reserved
    assert refused(w4=0b101)                                        # x[0]: a bit at column 2 >= w
    assert refused(w6=1)                                            # x[2]: a row >= h
    assert refused(w22=1) and refused(w41=1) and refused(w60=1)     # the last row of x, o, e
    assert refused(w23=1)                                           # o[0] on a cell x[0] holds
    assert refused(w43=1)                                           # e[1] on a cell o[1] holds
    assert refused(w42=0b11)                                        # e[0] on a cell x[0] holds
    table = np.zeros(M.TABLE_WORDS, np.uint32)
    assert lib.sgo_shape_compile(S, None, L.ptr(table)) == SGO_ERR_ARG
    assert lib.sgo_shape_compile(S, L.ptr(good), None) == SGO_ERR_ARG


def test_parse_round_trips_and_errors():
    Sh = shapes_mod.Shape
    for name, sh in SC.shapes(S).items():
        mine = Sh([list(r) for r in sh.cells], sh.edges)
        again = Sh.parse(mine.text())
        assert (again.w, again.h, again.edges, again.cells) == (mine.w, mine.h, mine.edges, mine.cells), name
        assert model_shape(again) == sh
    a = Sh.parse("|X?|\n|O*|")
    assert (a.w, a.h, a.edges) == (2, 2, shapes_mod.L | shapes_mod.R) and a.cells == [[1, 0], [2, 0]]
    b = Sh.parse("X.\n O *\n+--")
    assert b.edges == shapes_mod.B and b.cells == [[1, 3], [2, 0]]
    assert Sh.parse("-\nX").edges == shapes_mod.T and Sh.parse("+-+/|X|/+-+").edges == 15
    assert Sh.parse(HOOK).cells == [[3, 1, 2], [0, 1, 3]]
    for bad in ("", "---", "|X.\nO*", "X.|\nO*", "X.\nO", "XA", "X#"):
        with pytest.raises(ValueError):
            Sh.parse(bad)
    # the sixteen variants are the model's, and to_base leads every cell back to the cell it shows
    hook = Sh.parse(HOOK)
    for var in hook.variants():
        want = M.variant(model_shape(hook), var.v)
        assert (var.w, var.h, var.edges, var.cells) == (want.w, want.h, want.edges, want.cells)
        for j in range(var.h):
            for i in range(var.w):
                bi, bj = var.to_base(i, j)
                k = hook.cells[bj][bi]
                assert var.cells[j][i] == (3 - k if var.c and k in (1, 2) else k)
    side = Sh.parse("|X.\n|O*")
    assert [v.edges for v in side.variants()[:8]] == [1, 2, 4, 1, 2, 4, 8, 8]


def _game(entries, n_setup=0):
    return SgfGame(S, 5.5, list(entries), [i < n_setup for i in range(len(entries))])


def _records():
    mk = lambda name, e, w: R.Record(name, S, list(e), [False] * len(e), list(range(1, len(e) + 1)), w)   # noqa: E731
    return [mk("a", GAME_A, -1), mk("b", GAME_B, None), mk("c", GAME_C, 1), mk("d", GAME_D, 1)]


def test_record_set_find():
    hook = shapes_mod.Shape.parse(HOOK)
    rs = R.RecordSet(_records(), S, backend=ShapesRecords(S, 8, 64))
    found = rs.find(hook)
    assert [c[0] for c in rs.backend.calls] == ["replay", "shapes"]
    assert found["searched"] == 4 and found["matched"] == 3
    by = {d["name"]: d for d in found["games"]}
    assert by["a"] == {"name": "a", "ply": 3, "variant": 0, "x0": 1, "y0": 1, "next": ("cell", 0, 0, "O")}
    assert by["d"]["ply"] == 3 and by["d"]["next"] == ("pass",)
    assert by["b"]["ply"] == 3 and by["b"]["variant"] >= 8 and by["b"]["next"] == ("elsewhere",)
    assert found["continuations"] == [
        {"key": ("cell", 0, 0, "O"), "label": "O(0,0)", "count": 1, "wins": 1, "losses": 0},
        {"key": ("elsewhere",), "label": "elsewhere", "count": 1, "wins": 0, "losses": 0},
        {"key": ("pass",), "label": "pass/end", "count": 1, "wins": 0, "losses": 0}]
    # the rows of the generator: one per record, the position after entry k in row base + k
    ch = next(rs.shapes(hook))
    assert ch.shapes.hits.shape == (sum(len(r.entries) + 1 for r in rs.records), 4)
    assert ch.shapes.first(3) == (0, 1, 1) and ch.shapes.n_hits(2) == 0 and ch.shapes.first(2) is None
    assert ch.shapes.cover(3) == sorted([P(1, 1), P(2, 1), P(3, 1), P(2, 2), P(3, 2)])
    assert ch.shapes.n_hits(4) == 0                                  # white sits on the cell that had to be empty


def test_continuation_in_every_variant():
    """a move on a cell of the shape comes back to the same cell of the shape as drawn, whichever variant matched"""
    hook = shapes_mod.Shape.parse(HOOK)
    for var in hook.variants():
        for j in range(var.h):
            for i in range(var.w):
                key = shapes_mod.continuation(hook, 9, (var.v, 2, 3), (3 + j) * 9 + 2 + i, 1)
                assert key == ("cell",) + var.to_base(i, j) + ("O" if var.c else "X",)
        assert shapes_mod.continuation(hook, 9, (var.v, 2, 3), 0, -1) == ("elsewhere",)
        assert shapes_mod.continuation(hook, 9, (var.v, 2, 3), 81, -1) == ("pass",)
        assert shapes_mod.continuation(hook, 9, (var.v, 2, 3), None, 0) == ("pass",)


def test_review_find_flags():
    hook = shapes_mod.Shape.parse(HOOK)
    game = _game(GAME_A)
    rec = R.Record("game", S, list(game.moves), list(game.setup), list(range(1, len(game.moves) + 1)), None)
    mk = lambda: R.RecordSet([rec], S, backend=ShapesRecords(S, 4, 64))                  # noqa: E731
    found = review.find_rows(game, mk(), hook)
    assert found == {1: {"hits": 0, "flags": []}, 2: {"hits": 0, "flags": []}, 3: {"hits": 1, "flags": ["appears"]},
                     4: {"hits": 0, "flags": ["disappears"]}, 5: {"hits": 0, "flags": []}}
    rows = [{"move_number": m, "colour": "B", "played": "A1", "played_share": 0.5, "played_mean": 0.1, "best": "B2", "best_mean": 0.2,
             "top": [{"pv": ["B2", "C3"]}]} for m in (1, 3, 4, 9)]
    plain = [review.format_row(dict(r)) for r in rows]
    review.add_find(rows, game, hook, record_set=mk())
    assert [r.get("find_flags") for r in rows] == [[], ["appears"], ["disappears"], None]
    assert [review.format_row(r) for r in rows] == [plain[0], plain[1] + "  | appears", plain[2] + "  | disappears", plain[3]]
    assert shapes_mod.review_flags(True, True) == [] and shapes_mod.review_flags(False, False) == []


def _sgf(entries, result=None):
    L = "abcde"
    pt = lambda a: "[]" if a >= S * S else "[%s]" % (L[a % S] + L[a // S])               # noqa: E731
    return "(;FF[4]SZ[5]KM[5.5]%s" % ("RE[%s]" % result if result else "") + \
        "".join(";%s%s" % ("B" if c > 0 else "W", pt(a)) for a, c in entries) + ")"


def test_records_find_lines(tmp_path, monkeypatch):
    for name, entries, result in (("a", GAME_A, "W+3.5"), ("b", GAME_B, None), ("c", GAME_C, "B+R"), ("d", GAME_D, "B+1.5")):
        (tmp_path / (name + ".sgf")).write_text(_sgf(entries, result))
    shape_file = tmp_path / "hook.txt"
    shape_file.write_text(".XO\n*X.\n")
    monkeypatch.setattr(R, "DeviceRecords", ShapesRecords)
    out, doc = io.StringIO(), tmp_path / "out.json"
    assert R.main([str(tmp_path), "--size", "5", "--find", str(shape_file), "--json", str(doc)], out=out) == 0
    lines = [l for l in out.getvalue().split("\n") if l.startswith("find ")]
    assert lines == ["find %s: games matched 3 / searched 4" % shape_file,
                     "find next O(0,0)     count 1 wins 1 losses 0",
                     "find next elsewhere  count 1 wins 0 losses 0",
                     "find next pass/end   count 1 wins 0 losses 0"]
    d = json.loads(doc.read_text())["find"]
    assert d["matched"] == 3 and d["searched"] == 4 and d["continuations"][0]["key"] == ["cell", 0, 0, "O"]


class ShapesEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `shapes` serves the model's row of a case"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self, size, case):
        names, recs = SC.case_records(size)
        self.size, self.rec = size, recs[names.index(case)][None]

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def shapes(self, shape):
        m = M.shapes(self.size, self.rec, model_shape(shape))
        return shapes_mod.Shapes(self.size, m["hits"], m["cover"])


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_find(conf5):
    e = gtp.GTPEngine(engine=ShapesEngine(S, "hook@1,1_b"))
    assert e.parse_command("known_command sgo-find") == "= true\n\n" and "sgo-find" in e.parse_command("list_commands").split()
    assert e.parse_command("sgo-find " + HOOK) == "= .....\n.###.\n..##.\n.....\n.....\nhits 1 variants 0 cover 5\n\n"
    assert e.parse_command("sgo_find " + HOOK) == e.parse_command("sgo-find " + HOOK)
    assert e.parse_command("sgo-find O").endswith("\nhits 3 variants 0,8 cover 3\n\n")      # one white stone as drawn, two black exchanged
    assert e.parse_command("sgo-find |X").endswith("\nhits 0 variants - cover 0\n\n")
    assert e.parse_command("sgo-find") == "? syntax error\n\n"
    assert e.parse_command("sgo-find XA").startswith("? bad shape")

    class Host(object):
        """the host engine's surface: no load, no shapes"""
        model = type("N", (), {"name": "x"})()

    assert gtp.GTPEngine(engine=Host()).parse_command("sgo-find X") == "? not supported\n\n"
