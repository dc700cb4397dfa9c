"""CPU model of the shape search (include/sgo.h "shape search"), written from the header's text on plain Python sets of points:
the sixteen variants by TRANSFORMING THE SHAPE cell by cell, the edge flags carried with the sides of the grid (derived from the
cell formulas on a probe grid, not copied from the header's last column), the drop of repeated variants, the match cell by cell at
every placement.  No code of the package takes part, and nothing of the kernel's (row masks, shifts, Horner) is used.  Everything
is integer: the GPU results must match word for word.

A shape here is `Shape(w, h, edges, cells)`, cells[j][i] in {DC, X, O, E}.  The match is stated per CELL: a placement (x0, y0)
matches iff every cell, don't-care included, lies on the board and finds what it asks for.  That is the header's "the window lies
on the board" and lets each off-board fault relax exactly one kind of cell.

FAULT SWITCHES -- each the kind of slip a kernel could hold (tests/test_shapes_model_power.py shows which case notices which).
Model and test helper only; no library code reads them.
  empty_off_board        a must-be-empty cell is satisfied beyond the board's edge (an empty mask that is not cut to the board)
  dontcare_off_board_x   a don't-care cell may lie beyond the left / right edge (no x0 <= S - w' in the placement mask)
  dontcare_off_board_y   a don't-care cell may lie beyond the top / bottom edge (no y0 <= S - h' in the placement mask)
  flag_as_stone          the to-play flag is read as a black stone
  history_read           planes 2 / 3 (the position one ply ago) are read as stones as well
  padding_read           bits >= N of planes 0 / 1 (other than the flag) are read as stones
  edges_ignored          the edge flags are dropped
  edges_not_moved        a variant keeps the edge flags of the shape as drawn
  no_colour_swap         only the eight variants with c = 0 exist
  duplicates_counted     no variant is dropped
  rot_labels_swapped     the two rotations carry each other's number (g = 4 <-> g = 6)
  first_not_lowest       `first` is the largest code among the matches
  cover_has_dontcare     the cover holds the points under don't-care cells too

With flag_as_stone / padding_read the position is taken on the STRIP the plane words form (width S, 32 * NW points), as a kernel
reading the words without a mask would see it; the output words then carry what the strip holds."""
import collections

import numpy as np

FAULTS = ("empty_off_board", "dontcare_off_board_x", "dontcare_off_board_y", "flag_as_stone", "history_read", "padding_read",
          "edges_ignored", "edges_not_moved", "no_colour_swap", "duplicates_counted", "rot_labels_swapped", "first_not_lowest",
          "cover_has_dontcare")
SIZES = (5, 7, 9, 13, 19)
DC, X, O, E = 0, 1, 2, 3
L, T, R, B = 1, 2, 4, 8
TABLE_WORDS = 16 + 16 * 64

Shape = collections.namedtuple("Shape", "w h edges cells")


def shape(rows, edges=0):
    """Shape of an ASCII picture: X, O, `.` must be empty, `*` don't-care"""
    rows = [r.replace(" ", "") for r in rows]
    assert rows and all(len(r) == len(rows[0]) for r in rows)
    return Shape(len(rows[0]), len(rows), edges, tuple(tuple({"X": X, "O": O, ".": E, "*": DC}[ch] for ch in r) for r in rows))


def source(g, i, j, w, h):
    """(row, column) of the cell of the w x h grid that cell (i, j) of variant g shows: the header's eight formulas"""
    return ((j, i), (i, j), (j, w - 1 - i), (h - 1 - j, i), (h - 1 - i, j), (h - 1 - j, w - 1 - i), (i, w - 1 - j), (h - 1 - i, w - 1 - j))[g]


def dims(g, w, h):
    return (h, w) if g in (1, 4, 6, 7) else (w, h)


def edge_sources(g):
    """{new side: old side}: where the four sides of variant g's grid come from, found on a 3 x 4 probe (every side a different
    length or position, so nothing is ambiguous): the side of the new grid is the line of cells that lay on that old side"""
    w, h = 3, 4
    w2, h2 = dims(g, w, h)
    old = {L: {(j, 0) for j in range(h)}, R: {(j, w - 1) for j in range(h)}, T: {(0, i) for i in range(w)}, B: {(h - 1, i) for i in range(w)}}
    new = {L: [(0, j) for j in range(h2)], R: [(w2 - 1, j) for j in range(h2)], T: [(i, 0) for i in range(w2)], B: [(i, h2 - 1) for i in range(w2)]}
    out = {}
    for side, cells in new.items():
        got = {source(g, i, j, w, h) for i, j in cells}
        out[side] = [s for s, line in old.items() if line == got][0]
    return out


def variant(sh, v, fault=None):
    """the Shape of variant v = 8 c + g"""
    g, c = v & 7, v >> 3
    w2, h2 = dims(g, sh.w, sh.h)
    swap = {DC: DC, E: E, X: O, O: X} if c else {DC: DC, E: E, X: X, O: O}
    cells = []
    for j in range(h2):
        row = []
        for i in range(w2):
            sj, si = source(g, i, j, sh.w, sh.h)
            row.append(swap[sh.cells[sj][si]])
        cells.append(tuple(row))
    edges = 0
    for side, frm in edge_sources(g).items():
        if sh.edges & frm:
            edges |= side
    if fault == "edges_not_moved":
        edges = sh.edges
    if fault == "edges_ignored":
        edges = 0
    return Shape(w2, h2, edges, tuple(cells))


def kept_variants(sh, fault=None):
    """[(v, Shape)] in ascending v, a variant equal to an earlier one dropped"""
    out = []
    for v in range(8 if fault == "no_colour_swap" else 16):
        s = variant(sh, v, fault)
        if fault != "duplicates_counted" and any(s == k for _, k in out):
            continue
        out.append((v, s))
    if fault == "rot_labels_swapped":
        relabel = {4: 6, 6: 4, 12: 14, 14: 12}
        out = sorted((relabel.get(v, v), s) for v, s in out)
    return out


def struct_words(sh):
    """the sgo_shape of a Shape as 61 32-bit words: w, h, edges, reserved, x[19], o[19], e[19]"""
    out = np.zeros(4 + 3 * 19, np.uint32)
    out[0], out[1], out[2] = sh.w, sh.h, sh.edges
    for j, row in enumerate(sh.cells):
        for i, c in enumerate(row):
            if c != DC:
                out[4 + 19 * (c - 1) + j] |= np.uint32(1 << i)
    return out


def table(S, sh):
    """what sgo_shape_compile writes for a shape it accepts"""
    t = np.zeros(TABLE_WORDS, np.uint32)
    kept = kept_variants(sh)
    t[:6] = [S, len(kept), sum(1 << v for v, _ in kept), sh.w, sh.h, sh.edges]
    for k, (v, s) in enumerate(kept):
        slot = t[16 + 64 * k:16 + 64 * (k + 1)]
        slot[:4] = [v, s.w, s.h, s.edges]
        slot[4:61] = struct_words(s)[4:]
    return t


def _bits(words):
    return [int(a) for a in np.flatnonzero(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little"))]


def record_stones(S, rec, fault=None):
    """(black, white, area): the stones of a packed record as sets of points, and how many points the position has"""
    N, NW = S * S, (S * S + 31) // 32
    p = np.asarray(rec, dtype=np.uint32).reshape(16, NW)
    black, white = _bits(p[0]), _bits(p[1])
    flag = 32 * NW - 1
    if fault == "padding_read":
        black = [a for a in black if a != flag]
        return set(black), set(a for a in white if a not in black), 32 * NW
    if fault == "flag_as_stone":
        return set(a for a in black if a < N or a == flag), set(a for a in white if a < N), 32 * NW
    black, white = set(a for a in black if a < N), set(a for a in white if a < N)
    if fault == "history_read":
        black |= set(a for a in _bits(p[2]) if a < N) - white
        white |= set(a for a in _bits(p[3]) if a < N) - black
    return black, white, N


def point_shapes(S, black, white, sh, fault=None, area=None):
    """(hits [n_hits, first, vmask, n_cover], cover set of points, matches [(v, x0, y0)]) of one position given as point sets"""
    area = S * S if area is None else area
    rows = (area + S - 1) // S
    black, white = set(black), set(white)

    def on(x, y):
        return 0 <= x < S and y >= 0 and y * S + x < area

    # without a fault that lets a cell pass off the board, a window that leaves the board fails on its first cell outside: those
    # placements are not walked at all (the model's speed, not its meaning)
    wide = fault in ("empty_off_board", "dontcare_off_board_x", "dontcare_off_board_y") or area != S * S
    matches, cover = [], set()
    for v, s in kept_variants(sh, fault):
        for y0 in (range(-s.h + 1, rows) if wide else range(0, S - s.h + 1)):
            for x0 in (range(-s.w + 1, S) if wide else range(0, S - s.w + 1)):
                if (s.edges & L and x0 != 0) or (s.edges & T and y0 != 0) or (s.edges & R and x0 + s.w != S) or (s.edges & B and y0 + s.h != S):
                    continue
                good, under = True, set()
                for j in range(s.h):
                    for i in range(s.w):
                        c, x, y = s.cells[j][i], x0 + i, y0 + j
                        a = y * S + x
                        if on(x, y):
                            fine = c == DC or (c == X and a in black) or (c == O and a in white) or (c == E and a not in black and a not in white)
                            if c != DC or fault == "cover_has_dontcare":
                                under.add(a)
                        elif c == E:
                            fine = fault == "empty_off_board"
                        elif c == DC:
                            x_in, y_in = 0 <= x < S, 0 <= y < rows
                            fine = (fault == "dontcare_off_board_x" and y_in and not x_in) or (fault == "dontcare_off_board_y" and x_in and not y_in)
                        else:
                            fine = False
                        if not fine:
                            good = False
                            break
                    if not good:
                        break
                if good:
                    matches.append((v, x0, y0))
                    cover |= under
    codes = [(v * S + y0) * S + x0 for v, x0, y0 in matches]
    first = -1 if not codes else (max(codes) if fault == "first_not_lowest" else min(codes))
    vmask = 0
    for v, _, _ in matches:
        vmask |= 1 << v
    return [len(matches), first, vmask, len(cover)], cover, matches


def placements(S, sh):
    """[(v, x0, y0, black, white, empty, under)]: every placement of every kept variant that lies on the board and touches its
    edges, with the points it needs black / white / empty and the points under its cared cells -- the header's match taken apart
    so that many positions can be asked at once (tests/test_shapes_model_power.py ties it to point_shapes)"""
    out = []
    for v, s in kept_variants(sh):
        for y0 in range(0, S - s.h + 1):
            for x0 in range(0, S - s.w + 1):
                if (s.edges & L and x0 != 0) or (s.edges & T and y0 != 0) or (s.edges & R and x0 + s.w != S) or (s.edges & B and y0 + s.h != S):
                    continue
                need = {X: [], O: [], E: []}
                for j in range(s.h):
                    for i in range(s.w):
                        if s.cells[j][i] != DC:
                            need[s.cells[j][i]].append((y0 + j) * S + x0 + i)
                out.append((v, x0, y0, need[X], need[O], need[E], sorted(need[X] + need[O] + need[E])))
    return out


def _words(pts, NW):
    w = np.zeros(NW, np.uint32)
    for a in pts:
        w[a >> 5] |= np.uint32(1 << (a & 31))
    return w


def record_shapes(S, rec, sh, fault=None):
    """(hits int32 [4], cover uint32 [NW]) of one packed record"""
    black, white, area = record_stones(S, rec, fault)
    hits, cover, _ = point_shapes(S, black, white, sh, fault, area)
    return np.array(hits, np.int32), _words(cover, (S * S + 31) // 32)


def shapes(S, records, sh, index=None, fault=None):
    """The outputs of sgo_shapes_dev for n rows: {"hits" int32 [n, 4], "cover" uint32 [n, NW]}.  records uint32 [R, 16 * NW]; index
    None = rows 0 .. R - 1; a row outside [0, R) gives {0, -1, 0, 0} and a zero cover."""
    records = np.asarray(records, dtype=np.uint32)
    Rn, NW = len(records), (S * S + 31) // 32
    index = np.arange(Rn) if index is None else np.asarray(index, dtype=np.int64)
    n = len(index)
    out = {"hits": np.zeros((n, 4), np.int32), "cover": np.zeros((n, NW), np.uint32)}
    out["hits"][:, 1] = -1
    cache = {}
    for i, r in enumerate(index):
        r = int(r)
        if r < 0 or r >= Rn:
            continue
        if r not in cache:
            cache[r] = record_shapes(S, records[r], sh, fault)
        out["hits"][i], out["cover"][i] = cache[r]
    return out


def build_record(S, black, white, white_to_play, rng=None):
    """uint32 [16 * NW]: planes 0 / 1 the stones.  With rng: random words in planes 2..15 and in the padding bits of planes 0 / 1
    (the flag is set as asked)."""
    N, NW = S * S, (S * S + 31) // 32
    rec = np.zeros((16, NW), np.uint32)
    if rng is not None:
        rec[:] = rng.randint(0, 1 << 32, size=(16, NW), dtype=np.uint64).astype(np.uint32)
        live = np.zeros(32 * NW, bool)
        live[:N] = True
        livew = np.packbits(live, bitorder="little").view("<u4").astype(np.uint32)
        rec[:2] &= ~livew
        rec[0, NW - 1] &= np.uint32(0x7fffffff)
    for plane, pts in enumerate((black, white)):
        for a in pts:
            rec[plane, a >> 5] |= np.uint32(1 << (a & 31))
    if white_to_play:
        rec[0, NW - 1] |= np.uint32(0x80000000)
    return rec.reshape(-1)


def points_of(words, N):
    """the points a < N of a bitset"""
    return [a for a in _bits(words) if a < N]
