"""Shape search on the device (include/sgo.h "shape search", csrc/sgo_shapes.hip): where does a local pattern of black / white /
empty / don't-care cells occur in a position, in any of its sixteen variants (eight symmetries, colours as drawn or exchanged),
anchored to the board edges it names -- and, over a game collection, what was played next.

    from sejonggo_amd.shapes import Shape, shapes
    sh = Shape.parse('''
        +-----
        |.....
        |..XO.
        |..X..
    ''')                                     # X O . and * (or ?) for don't-care; | and - / + lines anchor the grid to the edges
    v = shapes(19, records, sh)              # packed records uint32 [R, 16 * NW], host or device
    v.n_hits(0), v.first(0), v.cover(0)

records.RecordSet.find(shape) searches a game collection and tallies the continuations, engine.SessionEngine.shapes(slots, shape)
reads session slots; GTP's `sgo-find`, `python -m sejonggo_amd.records DIR --find SHAPE.txt` and `python -m sejonggo_amd.review
game.sgf --find SHAPE.txt` stand on them."""
import collections
import ctypes as C

import numpy as np

from ._packed import device_records, points as _points

DC, X, O, E = 0, 1, 2, 3
L, T, R, B = 1, 2, 4, 8
_CHARS = {"X": X, "O": O, ".": E, "*": DC, "?": DC}
_TEXT = {X: "X", O: "O", E: ".", DC: "*"}
# new L, T, R, B = old ..., per g (include/sgo.h)
_EDGE_FROM = ((L, T, R, B), (T, L, B, R), (R, T, L, B), (L, B, R, T), (B, L, T, R), (R, B, L, T), (T, R, B, L), (B, R, T, L))


class ShapeStruct(C.Structure):
    """sgo_shape of include/sgo.h"""
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("edges", C.c_int32), ("reserved", C.c_int32),
                ("x", C.c_uint32 * 19), ("o", C.c_uint32 * 19), ("e", C.c_uint32 * 19)]


def _source(g, i, j, w, h):
    """(row, column) of the base cell that cell (i, j) of variant g shows"""
    return ((j, i), (i, j), (j, w - 1 - i), (h - 1 - j, i), (h - 1 - i, j), (h - 1 - j, w - 1 - i), (i, w - 1 - j), (h - 1 - i, w - 1 - j))[g]


class Variant(collections.namedtuple("Variant", "v c g w h edges cells base_w base_h")):
    """Variant v = 8 c + g of a shape: its own grid, and the way back to the grid as drawn"""

    def to_base(self, i, j):
        """(column, row) of the cell of the shape as drawn that cell (i, j) of this variant shows; `c` tells whether the colours
        were exchanged on the way"""
        sj, si = _source(self.g, i, j, self.base_w, self.base_h)
        return si, sj


class Shape(object):
    """cells[j][i] in {DC, X, O, E}, row j from the top, column i from the left; edges a bit set of L, T, R, B"""

    def __init__(self, cells, edges=0):
        self.cells = [list(row) for row in cells]
        self.h, self.w, self.edges = len(self.cells), len(self.cells[0]) if self.cells else 0, int(edges)
        if not self.h or not self.w or any(len(r) != self.w for r in self.cells):
            raise ValueError("a shape is a rectangle of at least one cell")
        if self.w > 19 or self.h > 19 or not 0 <= self.edges <= 15 or any(c not in (DC, X, O, E) for r in self.cells for c in r):
            raise ValueError("a shape has at most 19 x 19 cells of X O . * and edges in [0, 15]")

    @classmethod
    def parse(cls, text):
        """Rows of `X O . *` (`?` = `*`; blanks inside a row are ignored).  A leading / trailing `|` on EVERY row anchors the grid
        to the left / right edge; a first / last line of `-` (corners `+`, or `|`) anchors it to the top / bottom edge."""
        lines = [ln.strip().replace(" ", "") for ln in text.replace("/", "\n").split("\n")]
        lines = [ln for ln in lines if ln]
        edges = 0
        border = lambda ln: set(ln) <= set("-+|") and "-" in ln                          # noqa: E731
        if lines and border(lines[0]):
            edges |= T
            lines = lines[1:]
        if lines and border(lines[-1]):
            edges |= B
            lines = lines[:-1]
        if not lines:
            raise ValueError("a shape needs at least one row")
        for side, at in ((L, 0), (R, -1)):
            have = [ln[at] == "|" for ln in lines]
            if any(have) and not all(have):
                raise ValueError("`|` must stand on every row or on none")
            if all(have):
                edges |= side
                lines = [ln[1:] if side == L else ln[:-1] for ln in lines]
        if any(not ln for ln in lines) or any(len(ln) != len(lines[0]) for ln in lines):
            raise ValueError("the rows of a shape have one length")
        bad = sorted(set(ch for ln in lines for ch in ln) - set(_CHARS))
        if bad:
            raise ValueError("a shape is drawn with X O . * ?, not %r" % "".join(bad))
        return cls([[_CHARS[ch] for ch in ln] for ln in lines], edges)

    def text(self):
        """the picture `parse` reads back"""
        rows = ["".join(_TEXT[c] for c in r) for r in self.cells]
        rows = [("|" if self.edges & L else "") + r + ("|" if self.edges & R else "") for r in rows]
        bar = "+" + "-" * (len(rows[0]) - 1) if len(rows[0]) > 1 else "-"
        return "\n".join(([bar] if self.edges & T else []) + rows + ([bar] if self.edges & B else []))

    def to_struct(self):
        s = ShapeStruct()
        s.w, s.h, s.edges, s.reserved = self.w, self.h, self.edges, 0
        for j, row in enumerate(self.cells):
            for i, c in enumerate(row):
                if c == X:
                    s.x[j] |= 1 << i
                elif c == O:
                    s.o[j] |= 1 << i
                elif c == E:
                    s.e[j] |= 1 << i
        return s

    def variants(self):
        """the sixteen Variants, v = 0 .. 15 (repeated ones included: the device drops a variant equal to an earlier one)"""
        out = []
        for v in range(16):
            g, c = v & 7, v >> 3
            w2, h2 = (self.h, self.w) if g in (1, 4, 6, 7) else (self.w, self.h)
            cells = []
            for j in range(h2):
                row = []
                for i in range(w2):
                    sj, si = _source(g, i, j, self.w, self.h)
                    k = self.cells[sj][si]
                    row.append(3 - k if c and k in (X, O) else k)
                cells.append(tuple(row))
            edges = sum(new for new, old in zip((L, T, R, B), _EDGE_FROM[g]) if self.edges & old)
            out.append(Variant(v, c, g, w2, h2, edges, tuple(cells), self.w, self.h))
        return out


def compile_table(size, shape):
    """uint32 [SGO_SHAPE_TABLE_WORDS]: sgo_shape_compile's table of a Shape (host arithmetic; no device)"""
    from . import _lib
    lib = _lib.load()
    table = np.zeros(16 + 16 * 64, np.uint32)
    s = shape.to_struct()
    _lib.check(lib.sgo_shape_compile(C.c_int(size), C.byref(s), _lib.ptr(table)), "sgo_shape_compile")
    return table


class Shapes(object):
    """hits int32 [n, 4] (n_hits, first, vmask, n_cover), cover uint32 [n, NW]"""

    def __init__(self, size, hits, cover):
        self.S, self.N = size, size * size
        self.hits, self.cover_words = np.asarray(hits, dtype=np.int32), np.asarray(cover, dtype=np.uint32)

    def __len__(self):
        return len(self.hits)

    def n_hits(self, i):
        return int(self.hits[i, 0])

    def first(self, i):
        """(v, x0, y0) of the lowest match, None without one"""
        code = int(self.hits[i, 1])
        if code < 0:
            return None
        return code // self.N, code % self.S, (code % self.N) // self.S

    def variants(self, i):
        return [v for v in range(16) if (int(self.hits[i, 2]) >> v) & 1]

    def cover(self, i):
        """the board points under cared cells of any match"""
        return _points(self.cover_words[i], self.N)


def shapes(size, records, shape, index=None):
    """sgo_shapes_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Shapes with one row per
    entry of `index` (None: every record in order); an index outside [0, R) gives {0, -1, 0, 0} and an empty cover."""
    import torch
    from . import _lib
    records, Rn, idx, n = device_records(size, records, index)
    lib, dev = _lib.load(), records.device
    table = torch.from_numpy(compile_table(size, shape).view(np.int32)).to(dev)
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    cover = torch.zeros((n, lib.sgo_plane_words(size)), dtype=torch.int32, device=dev)
    _lib.check(lib.sgo_shapes_dev(C.c_int(size), C.c_int(n), _lib.ptr(records), C.c_int(Rn), _lib.ptr(idx), _lib.ptr(table), _lib.ptr(hits),
                                  _lib.ptr(cover), _lib.stream_ptr()), "sgo_shapes_dev")
    return Shapes(size, hits.cpu().numpy(), cover.cpu().numpy().view(np.uint32))


def format_cover(v, i=0):
    """`sgo-find` text of row i of a Shapes: S lines of S characters from the top row down -- # a point under a cared cell of a
    match, . anything else -- then `hits H variants V cover K` (V = the matching variants, or -)."""
    S = v.S
    text = ["."] * v.N
    for a in v.cover(i):
        text[a] = "#"
    lines = ["".join(text[y * S:(y + 1) * S]) for y in range(S)]
    lines.append("hits %d variants %s cover %d" % (v.n_hits(i), ",".join("%d" % k for k in v.variants(i)) or "-", int(v.hits[i, 3])))
    return "\n".join(lines)


# ---- what was played next: a move of the game in the frame of the shape as drawn ------------------------------------------------------
def continuation(shape, size, first, action, colour):
    """Where the move (action, colour) lies relative to the match `first` = (v, x0, y0) of `shape`:
    ("cell", i, j, side)  on cell (i, j) of the shape as drawn, played by the side drawn as X or as O (side "X" / "O");
    ("elsewhere",)        a point outside the window;
    ("pass",)             a pass, or no move at all (action None: the game ended there)."""
    if action is None or action < 0 or action >= size * size:
        return ("pass",)
    v, x0, y0 = first
    var = shape.variants()[v]
    i, j = action % size - x0, action // size - y0
    if not (0 <= i < var.w and 0 <= j < var.h):
        return ("elsewhere",)
    bi, bj = var.to_base(i, j)
    side = "X" if (colour > 0) != bool(var.c) else "O"
    return ("cell", bi, bj, side)


def continuation_label(key):
    if key[0] == "cell":
        return "%s(%d,%d)" % (key[3], key[1], key[2])
    return "elsewhere" if key[0] == "elsewhere" else "pass/end"


# ---- game review: the plies at which the shape first appears and disappears ---------------------------------------------------------
def review_flags(present_before, present_after):
    """Flags of one move from whether the shape occurs in the position in front of it and in the one behind it: `appears` /
    `disappears`"""
    flags = []
    if present_after and not present_before:
        flags.append("appears")
    if present_before and not present_after:
        flags.append("disappears")
    return flags
