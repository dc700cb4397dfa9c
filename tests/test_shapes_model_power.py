"""CPU: what stands behind the shape-search model (tests/shapes_model.py).

1. The model transforms the SHAPE.  A second formulation here transforms the BOARD: it moves the stones with the eight
   sgo_sym_lut tables, matches only the shape as drawn and its colour exchange (variants c * 8 + 0) on the moved board, and carries
   every match back.  Two matches are one when they ask the same of the same points (window, cells, anchored sides): that is the
   header's drop of repeated variants, stated without variant numbers.  Both formulations give the same n_hits and the same cover
   for every shape of tests/shapes_cases.py on all 19 683 positions of a 3x3 corner of the 5x5 board and on a seeded 9x9 sample.
2. Every fault switch of the model is noticed by its named case of tests/shapes_cases.py, at every size.
3. The variant table of include/sgo.h: eight distinct grids on a 3 x 4 probe, closed under composition, and the edge column of
   the header equals what the cell formulas carry."""
import itertools

import numpy as np
import pytest

from tests import shapes_cases as SC
from tests import shapes_model as M

# the header's last column: new L, T, R, B = old ...
HEADER_EDGES = {0: "LTRB", 1: "TLBR", 2: "RTLB", 3: "LBRT", 4: "BLTR", 5: "RBLT", 6: "TRBL", 7: "BRTL"}
SIDE = {"L": M.L, "T": M.T, "R": M.R, "B": M.B}
NORMAL = {M.L: (-1, 0), M.T: (0, -1), M.R: (1, 0), M.B: (0, 1)}


def test_the_eight_formulas_and_the_edge_column():
    probe = M.Shape(3, 4, 0, tuple(tuple(range(4 * j, 4 * j + 3)) for j in range(4)))    # twelve distinct "cells"
    grids = []
    for g in range(8):
        w2, h2 = M.dims(g, 3, 4)
        grids.append(tuple(tuple(probe.cells[M.source(g, i, j, 3, 4)[0]][M.source(g, i, j, 3, 4)[1]] for i in range(w2)) for j in range(h2)))
    assert len(set(grids)) == 8

    def again(grid, g):
        h, w = len(grid), len(grid[0])
        w2, h2 = M.dims(g, w, h)
        return tuple(tuple(grid[M.source(g, i, j, w, h)[0]][M.source(g, i, j, w, h)[1]] for i in range(w2)) for j in range(h2))

    for a, b in itertools.product(range(8), repeat=2):
        assert again(grids[a], b) in grids                           # closed under composition
    for g in range(8):
        src = M.edge_sources(g)
        assert [src[s] for s in (M.L, M.T, M.R, M.B)] == [SIDE[ch] for ch in HEADER_EDGES[g]], g


def test_dedup_masks():
    sh = SC.shapes(5)
    kept = lambda name: sum(1 << v for v, _ in M.kept_variants(sh[name]))               # noqa: E731
    assert kept("stone") == 0x0101 and kept("hook") == 0xFFFF
    assert kept("stone_dc") == 0x4747                                # X*, X over *, *X, * over X (g = 0, 1, 2, 6), in both colours
    assert kept("pair") == 0x0303                                    # XX, its transpose, and the same in white
    assert kept("corner") == 0x2D2D                                  # its own transpose: g = 0, 2, 3, 5 -- one per corner
    assert kept("rows3") == 0x001B                                   # X*O down, across, and both reversed: the exchange is the flip


def _luts(S):
    from sejonggo_amd import symmetry
    return [np.asarray(symmetry.sym_lut(S, k))[:S * S].astype(np.int64) for k in range(8)]


def _by_shape(S, sh, black, white):
    """n_hits int [P], cover bool [P, N] from the model's placements: formulation one"""
    hits, cover = np.zeros(len(black), np.int64), np.zeros(black.shape, bool)
    occupied = black | white
    for v, x0, y0, nb, nw, ne, under in M.placements(S, sh):
        hit = black[:, nb].all(axis=1) & white[:, nw].all(axis=1) & ~occupied[:, ne].any(axis=1)
        hits += hit
        cover[:, under] |= hit[:, None]
    return hits, cover


def _by_board(S, sh, black, white):
    """the same from moved boards: formulation two"""
    N = S * S
    reps = {}
    for k, lut in enumerate(_luts(S)):
        inv = np.argsort(lut)                                        # inv[L[a]] = a: the moved point b came from inv[b]
        xy = lambda a: np.array([a % S, a // S])                                         # noqa: E731
        back = {}
        for side, (dx, dy) in NORMAL.items():                        # the side of the original board a moved side lies on
            d = xy(inv[(1 + dy) * S + 1 + dx]) - xy(inv[S + 1])
            back[side] = [s for s, n in NORMAL.items() if n == (int(d[0]), int(d[1]))][0]
        for c in (0, 1):
            s = M.variant(sh, 8 * c)
            for y0 in range(S - s.h + 1):
                for x0 in range(S - s.w + 1):
                    if (s.edges & M.L and x0) or (s.edges & M.T and y0) or (s.edges & M.R and x0 + s.w != S) or (s.edges & M.B and y0 + s.h != S):
                        continue
                    cells = [(s.cells[j][i], (y0 + j) * S + x0 + i) for j in range(s.h) for i in range(s.w)]
                    ident = (frozenset(int(inv[p]) for _, p in cells), frozenset((int(inv[p]), kind) for kind, p in cells if kind != M.DC),
                             frozenset(back[side] for side in NORMAL if s.edges & side))
                    reps.setdefault(ident, (k, cells))
    hits, cover = np.zeros(len(black), np.int64), np.zeros(black.shape, bool)
    moved = {}
    for k, cells in reps.values():
        if k not in moved:
            inv = np.argsort(_luts(S)[k])
            moved[k] = (black[:, inv], white[:, inv], inv)           # the stone on a sits on L[a]
        mb, mw, inv = moved[k]
        hit = np.ones(len(black), bool)
        for kind, p in cells:
            if kind == M.X:
                hit &= mb[:, p]
            elif kind == M.O:
                hit &= mw[:, p]
            elif kind == M.E:
                hit &= ~(mb[:, p] | mw[:, p])
        hits += hit
        cover[:, [int(inv[p]) for kind, p in cells if kind != M.DC]] |= hit[:, None]
    assert N == black.shape[1]
    return hits, cover


def _corner_positions():
    """all 3^9 positions of the 3x3 corner of a 5x5 board"""
    S = 5
    digits = np.array(list(itertools.product(range(3), repeat=9)), np.int8)
    pts = [y * S + x for y in range(3) for x in range(3)]
    black, white = np.zeros((len(digits), S * S), bool), np.zeros((len(digits), S * S), bool)
    black[:, pts], white[:, pts] = digits == 1, digits == 2
    return black, white


@pytest.mark.parametrize("S", (5, 9))
def test_moving_the_board_agrees_with_moving_the_shape(S):
    if S == 5:
        black, white = _corner_positions()
        assert len(black) == 19683
    else:
        rng = np.random.RandomState(9)
        cells = rng.randint(0, 4, size=(400, S * S))
        black, white = cells == 1, cells == 2
    total = 0
    for name, sh in SC.shapes(S).items():
        h1, c1 = _by_shape(S, sh, black, white)
        h2, c2 = _by_board(S, sh, black, white)
        assert np.array_equal(h1, h2), name
        assert np.array_equal(c1, c2), name
        assert (c1.sum(axis=1)[h1 == 0] == 0).all()
        total += int(h1.sum())
    assert total > 10000                                             # the comparison is about matches, not about their absence


@pytest.mark.parametrize("S", (5, 9))
def test_placements_are_the_models_match(S):
    """the taken-apart form the comparison above uses gives what point_shapes gives, position by position"""
    rng = np.random.RandomState(S)
    cells = rng.randint(0, 3, size=(12, S * S))
    black, white = cells == 1, cells == 2
    for name, sh in SC.shapes(S).items():
        hits, cover = _by_shape(S, sh, black, white)
        for p in range(len(cells)):
            got, cov, _ = M.point_shapes(S, np.flatnonzero(black[p]).tolist(), np.flatnonzero(white[p]).tolist(), sh)
            assert got[0] == hits[p] and sorted(cov) == np.flatnonzero(cover[p]).tolist(), (name, p)


@pytest.mark.parametrize("S", M.SIZES)
def test_every_fault_is_noticed_by_its_named_case(S):
    names, recs = SC.case_records(S)
    sh = SC.shapes(S)
    assert sorted(SC.NOTICED_BY) == sorted(M.FAULTS)
    for fault, (case, shape_name) in SC.NOTICED_BY.items():
        k = names.index(case)
        good = M.record_shapes(S, recs[k], sh[shape_name])
        bad = M.record_shapes(S, recs[k], sh[shape_name], fault)
        assert not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])), (fault, case, good[0], bad[0])


def test_what_the_named_cases_hold():
    """the figures the cases were drawn for, at 5x5"""
    S = 5
    names, recs = SC.case_records(S)
    sh = SC.shapes(S)
    hits = lambda case, shape: M.record_shapes(S, recs[names.index(case)], sh[shape])[0].tolist()   # noqa: E731
    assert hits("one_stone_b", "stone") == [1, 2 * S + 1, 1, 1]
    assert hits("two_stones_b", "stone") == [2, S + 1, 1, 2]
    assert hits("corner@1,1_b", "corner") == [0, -1, 0, 0] and hits("corner@0,0_b", "corner")[0] >= 1
    assert hits("corner/g5@br_b", "corner")[2] & (1 << 5)
    assert hits("side@2,1_b", "side")[0] == 0 and hits("side/g1@2,0_b", "side")[2] == (1 << 1) | (1 << 12)
    assert hits("hook/g4_b", "hook")[2] == 1 << 4 and hits("hook/g6_b", "hook")[2] == 1 << 6
    assert hits("hook_swapped_b", "hook")[2] == 1 << 8
    assert hits("flag_corner_w", "stone") == hits("flag_corner_b", "stone")
    assert hits("empty_b", "stone") == [0, -1, 0, 0]
    assert hits("board_full_b", "board_full")[0] >= 1 and hits("board_full_no_b", "board_full")[:2] == [0, -1]
    assert hits("col_full_b", "col_full")[0] >= 1 and hits("row_full_b", "row_full")[0] == 2
