"""The case set of the shape-search tests: a handful of shapes, and constructed positions at the smallest size at which each slip
can show, each for both values of the to-play flag over random words in planes 2..15 and in the padding.
tests/test_shapes_model_power.py shows which named (position, shape) pair notices which fault switch of tests/shapes_model.py;
tests/test_gpu_shapes.py runs every shape over every record on the device.

Every position is drawn from the shapes themselves (`draw`), so a case says what it holds: `hook@1,1` is the hook as drawn with its
top-left cell on (1, 1); `hook/g4` is its variant 4."""
import functools

import numpy as np

from tests import shapes_model as M

SIZES = M.SIZES


@functools.lru_cache(maxsize=None)
def shapes(S):
    """{name: Shape}: the shapes of every test, the windows 1x1, Sx1, 1xS and SxS among them"""
    out = {
        "stone": M.shape(["X"]),                                     # 1 x 1; symmetric: two variants are kept (X, O)
        "gap": M.shape(["."]),                                       # every empty point, once: the empty mask itself
        "stone_dc": M.shape(["X*"]),                                 # a don't-care cell beside the stone: eight variants
        "stone_e": M.shape(["X."]),                                  # a must-be-empty cell beside the stone
        "pair": M.shape(["XX"]),                                     # several matches in one record: `first`
        "hook": M.shape([".XO", "*X."]),                             # all four kinds of cell, no symmetry: sixteen variants
        "corner": M.shape(["*X.", "XO.", "..."], M.L | M.T),         # anchored to a corner
        "side": M.shape(["X.", "O*"], M.L),                          # anchored to one edge
        "rows3": M.shape(["X", "*", "O"]),                           # three rows: at 19x19 across the lanes 15 | 16
        # the whole width, asymmetric, all four kinds of cell, anchored left and right: one placement per row and variant
        "row_full": M.shape(["X" + "*" * (S - 3) + "O."], M.L | M.R),
        # the whole height, don't-care but for the bottom cell: a match must not see rows beyond the board
        "col_full": M.shape(["*"] * (S - 1) + ["X"]),
        # the whole board: a stone in one corner, an empty point in the opposite one
        "board_full": M.shape(["X" + "*" * (S - 1)] + ["*" * S] * (S - 2) + ["*" * (S - 1) + "."]),
    }
    return out


def draw(S, sh, ox, oy):
    """(black, white) with the X / O cells of a Shape placed with its top-left cell on (ox, oy)"""
    black, white = [], []
    for j, row in enumerate(sh.cells):
        for i, c in enumerate(row):
            assert 0 <= ox + i < S and 0 <= oy + j < S
            if c in (M.X, M.O):
                (black if c == M.X else white).append((oy + j) * S + ox + i)
    return sorted(black), sorted(white)


@functools.lru_cache(maxsize=None)
def positions(S):
    """[(name, black, white)]"""
    sh = shapes(S)
    P = lambda x, y: y * S + x                                                           # noqa: E731
    out = [("empty", [], [])]
    out.append(("one_stone", [P(1, 2)], []))                        # duplicates_counted
    out.append(("two_stones", [P(1, 1), P(3, 2)], []))               # first_not_lowest
    out.append(("pair_twice", [P(0, 0), P(1, 0), P(2, 3), P(3, 3)], [P(4, 4)]))
    # a stone on the last point and one on the first: windows in the last column and the last row, and what lies beyond them
    out.append(("last_point", [P(S - 1, S - 1)], [P(0, 0)]))
    out.append(("last_column", [P(S - 1, 1)], []))
    out.append(("last_row", [P(2, S - 1)], []))
    # the to-play flag beside an empty last point
    out.append(("flag_corner", [P(0, 0), P(S - 2, S - 1)], [P(S - 1, S - 2)]))
    out.append(("hook@1,1",) + draw(S, sh["hook"], 1, 1))
    out.append(("hook@br",) + draw(S, sh["hook"], S - 3, S - 2))     # against the right and the bottom edge
    b, w = draw(S, sh["hook"], 1, 1)
    out.append(("hook_swapped", w, b))                               # no_colour_swap
    for g in (1, 2, 3, 4, 5, 6, 7):
        out.append(("hook/g%d" % g,) + draw(S, M.variant(sh["hook"], g), 1, 1))        # rot_labels_swapped: g4 alone, g6 alone
    out.append(("corner@0,0",) + draw(S, sh["corner"], 0, 0))
    out.append(("corner@1,1",) + draw(S, sh["corner"], 1, 1))        # edges_ignored: the pattern away from the corner
    out.append(("corner/g5@br",) + draw(S, M.variant(sh["corner"], 5), S - 3, S - 3))   # in the opposite corner
    out.append(("side@0,1",) + draw(S, sh["side"], 0, 1))
    out.append(("side@2,1",) + draw(S, sh["side"], 2, 1))            # off the edge: no match
    out.append(("side/g1@2,0",) + draw(S, M.variant(sh["side"], 1), 2, 0))             # edges_not_moved: on the TOP edge
    out.append(("side/g2@r",) + draw(S, M.variant(sh["side"], 2), S - 2, 2))           # on the right edge
    # the full-width row in row 1 and mirrored in the last row; a full column with its stone in the last row and in the first
    b1, w1 = draw(S, sh["row_full"], 0, 1)
    b2, w2 = draw(S, M.variant(sh["row_full"], 2), 0, S - 1)
    out.append(("row_full", sorted(b1 + b2), sorted(w1 + w2)))
    out.append(("col_full", [P(3, S - 1), P(0, 0)], [P(S - 1, 2)]))
    # every point of the first and of the last row black: what the other half of a wavefront must never see
    out.append(("top_row", [P(x, 0) for x in range(S)], []))
    out.append(("bottom_row", [P(x, S - 1) for x in range(S)], []))
    out.append(("board_full", [P(0, 0)], [P(1, 1)]))
    out.append(("board_full_no", [P(0, 0)], [P(S - 1, S - 1)]))
    # three-row windows that start in rows S - 5, S - 4, S - 3: at 19x19 rows 14, 15, 16 on either side of lane 16
    out.append(("rows3", [P(0, S - 5), P(2, S - 4), P(4, S - 3)], [P(0, S - 3), P(2, S - 2), P(4, S - 1)]))
    return out


@functools.lru_cache(maxsize=None)
def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW]): every position for both flag values (`_b` / `_w` to play) over a random pattern"""
    rng = np.random.RandomState(4000 * S + seed)
    names, recs = [], []
    for name, b, w in positions(S):
        for wtp in (False, True):
            names.append("%s_%s" % (name, "w" if wtp else "b"))
            recs.append(M.build_record(S, b, w, wtp, rng))
    return names, np.stack(recs)


@functools.lru_cache(maxsize=None)
def case_model(S, shape_name):
    """the model's outputs of one shape on case_records(S), computed once and shared (read only)"""
    return M.shapes(S, case_records(S)[1], shapes(S)[shape_name])


# fault switch -> the (position, shape) pair that notices it, at every size
NOTICED_BY = {
    "empty_off_board": ("last_column_b", "stone_e"),
    "dontcare_off_board_x": ("last_column_b", "stone_dc"),
    "dontcare_off_board_y": ("last_row_b", "stone_dc"),
    "flag_as_stone": ("flag_corner_w", "stone"),
    "history_read": ("empty_b", "stone"),
    "padding_read": ("empty_b", "stone"),
    "edges_ignored": ("corner@1,1_b", "corner"),
    "edges_not_moved": ("side/g1@2,0_b", "side"),
    "no_colour_swap": ("hook_swapped_b", "hook"),
    "duplicates_counted": ("one_stone_b", "stone"),
    "rot_labels_swapped": ("hook/g4_b", "hook"),
    "first_not_lowest": ("two_stones_b", "stone"),
    "cover_has_dontcare": ("hook@1,1_b", "hook"),
}
