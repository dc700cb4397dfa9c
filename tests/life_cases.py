"""The case set of the unconditional-life tests: constructed positions at the smallest size at which each can go wrong, each for
both values of the to-play flag and both colour assignments (`_sb`: as drawn, black to play; `_sw`: as drawn, white to play; `_cb`
/ `_cw`: colours swapped) over random words in planes 2..15 and in the padding, then the positions of rule_shapes_S*.npz and every
fourth position of the golden 19x19 records.  tests/test_life_model_power.py shows what each case reaches and which fault switch of
tests/life_model.py it notices; tests/test_gpu_life.py runs the same records on the device.

The 5x5 shapes are drawn once and placed at every size against the edges they use (top-left corner, or the bottom edge).  From
7x7 on `cascade` is the snake of single stones that share one-point eyes pairwise down the main diagonal with its head cut open:
the removal runs the length of the board, one pair of stones per pass, S passes in all (19 at 19x19, the longest row of the GPU
tests); `diagonal_alive` is the same snake intact.

SHARE WITH A NON-EMPTY ALIVE SET (the model's count on the committed files, pinned in test_life_model_power.py): the rule shapes
are late play-out positions with large walls -- 16 of 24 at 5x5, 24 of 24 at every other size; of the 412 golden 19x19 positions
(every fourth of five games) 86 have one (21 %), and a golden position takes 2.5 removal passes per colour on average, 5 at
most."""
import functools

import numpy as np

from tests import life_model as M
from tests.tactics_cases import diagram, golden_records, lattice, rule_shape_records

SIZES = M.SIZES

# 5x5 shapes, X as drawn.  Placed with their top-left corner at (0, 0) unless they use the bottom edge.
SHAPES = {
    # two one-point eyes that touch diagonally in the corner: alive; regions joined diagonally make them one
    "two_eyes": ([".XX..", "X.X..", "XXX.."], "top"),
    # one eye: not alive
    "one_eye": ([".X...", "XX..."], "top"),
    # chains A (left) and B (top right) touch nowhere and share the eyes (1,0) and (2,1): alive only together
    "shared": (["X.XX.", "XX.X.", ".XX.."], "top"),
    # one private eye each: neither is alive
    "private": ([".X...", "XX...", ".....", "...XX", "...X."], "top"),
    # the corner region of three points: (0,0) touches no stone, so the region is vital to no one; the eye at (3,1) is not enough
    "corner3": (["..XXX", ".XX.X", "XXXXX"], "top"),
    # the same with a white stone on the corner point: every EMPTY point touches the chain, vital; the stone is dead
    "dead_stone": (["O.XXX", ".XX.X", "XXXXX"], "top"),
    # a living wall along the bottom (eyes at (0,3) and (2,3), a stone on the last point): the open board above is a region that
    # survives and is no territory
    "wall": (["XXXXX", ".X.XX", "XXXXX"], "bottom"),
    # two eyes on the bottom edge, and the stones next to the last board point: what a strip without a mask would open
    "edge_eyes": (["XXXX.", ".X.X."], "bottom"),
    # a white stone without a liberty in the corner (an illegal record): its region has no empty point and is vital to no one
    "illegal_corner": (["OX.X.", "XXXX."], "top"),
}
# at 5x5 only: the whole board settled, both colours alive
SETTLED = [".XXO.", "XXXOO", ".XXO.", "XXXOO", "XXXOO"]


def diagonal(S, open_end):
    """Eyes on the main diagonal (k, k), single stones on (k + 1, k) and (k, k + 1): every stone touches two one-point eyes.  With
    open_end the corner (0, 0) holds a stone instead of an eye: its chain of three has one eye and goes in round one, the eye
    (1, 1) with it, and so on down the diagonal -- S - 1 rounds remove something, the last stones (which had two vital regions in
    round one) in round S - 1.  Without open_end every stone is alive."""
    pts = [k * S + k + 1 for k in range(S - 1)] + [(k + 1) * S + k for k in range(S - 1)]
    return sorted(pts + ([0] if open_end else []))


def block(S, x0, y0):
    """a 5 x 3 block with eyes at (x0 + 1, y0 + 1) and (x0 + 3, y0 + 1)"""
    return [(y0 + dy) * S + x0 + dx for dy in range(3) for dx in range(5) if not (dy == 1 and dx in (1, 3))]


@functools.lru_cache(maxsize=None)
def positions(S):
    """[(name, black, white)] as drawn"""
    out = [("empty", [], [])]
    for name, (rows, edge) in SHAPES.items():
        b, w = diagram(S, rows, 0, S - len(rows) if edge == "bottom" else 0)
        out.append((name, b, w))
    if S == 5:
        b, w = diagram(S, SETTLED)
        out.append(("settled", b, w))
    if S >= 7:
        out.append(("cascade", diagonal(S, True), []))
        out.append(("diagonal_alive", diagonal(S, False), []))
    if S == 19:
        # stones and eyes across the word boundaries: eyes on 31 and 33 around a stone on 32; eyes on 63 and 65 around a stone on 64
        # (white); a stone on 360 beside the eyes 358 and 356
        out.append(("word_bounds", sorted(block(S, 11, 0) + block(S, 14, 16)), sorted(block(S, 5, 2))))
        b, w = lattice(S)
        out.append(("lattice", b, w))
        # a black stone without a liberty inside a living white group (an illegal record): its region is no eye and no territory
        b, w = diagram(S, ["OOOOOOO", "O.OXO.O", "OOOOOOO"], 3, 5)
        out.append(("illegal", b, w))
    return out


@functools.lru_cache(maxsize=None)
def case_points(S):
    """[(name, black, white, white to play)]: every position as drawn and with the colours swapped, for both flag values"""
    out = []
    for name, b, w in positions(S):
        for swap in (False, True):
            for wtp in (False, True):
                bb, ww = (w, b) if swap else (b, w)
                out.append(("%s_%s%s" % (name, "c" if swap else "s", "w" if wtp else "b"), list(bb), list(ww), wtp))
    return out


@functools.lru_cache(maxsize=None)
def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW]): the constructed positions over a random pattern, then the rule shapes"""
    rng = np.random.RandomState(3000 * S + seed)
    names, recs = [], []
    for name, b, w, wtp in case_points(S):
        names.append(name)
        recs.append(M.build_record(S, b, w, wtp, rng))
    shapes = rule_shape_records(S)
    names += ["shape_%d" % i for i in range(len(shapes))]
    return names, np.concatenate([np.stack(recs), shapes])


@functools.lru_cache(maxsize=None)
def case_model(S):
    """the model's outputs on case_records(S), computed once and shared (read only)"""
    return M.life(S, case_records(S)[1])


@functools.lru_cache(maxsize=None)
def golden_model():
    return M.life(19, golden_records())
