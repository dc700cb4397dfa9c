"""The case set of the influence tests: constructed positions, each as drawn with black to play (`_sb`) and with the colours
swapped and white to play (`_cw`), over random words in planes 2..15 and in the padding; each with the `dead` bitset it is run with
(None for most).  tests/test_influence_model_power.py shows which fault switch of tests/influence_model.py each named case
notices; tests/test_gpu_influence.py runs the same records on the device at the five parameter triples of M.TRIPLES.

  empty        nothing; with the flag set it is what shows a flag read as a stone (5x5: the flag lies two rows under the board)
  lone_centre  one stone on the centre point: no territory from 7x7 on, the whole board at 5x5
  lone_34      one stone on the 3-4 point (a = 2 S + 3), from 7x7 on
  lone_44      one stone on the 4-4 point, from 9x9 on
  corners      black on (2, 2), white on (S - 3, S - 3) (5x5: (1, 1) and (3, 3))
  full         every point black: 160 after eight dilations, and no erosion at all (no neighbour is <= 0: off-board ones do not count)
  contact      black (c, c) and (c, c + 1), white (c + 1, c): an opponent's value next to a point stops its dilation
  last_lines   black on the whole last row but its last point, white on the last column above it: what padding rows and the missing
               column S would change
  right_edge   a black stone on the last column, a white one on the first column two rows down: what a column wrap would join
  walls        black on row 1, white on row S - 2: territory behind both
  dead_inside  black on row 2, white on row S - 2, a white stone at (1, 0) behind black's wall and a black one at (S - 2, S - 1)
               behind white's; run with dead = those two stones, two empty points ((3, 0) and (S - 1, S - 1)) and stray bits >= N
  half_split   the left half black, the right half white, one empty column between (nothing at 5x5 but columns 0-1 / 3-4): long
               fronts, where erosion works on every step
"""
import functools

import numpy as np

from tests import influence_model as M
from tests.life_model import build_record
from tests.tactics_cases import golden_records, rule_shape_records

SIZES = M.SIZES


@functools.lru_cache(maxsize=None)
def positions(S):
    """[(name, black, white, dead points or None)] as drawn"""
    P = lambda x, y: y * S + x                                                           # noqa: E731
    c, N = S // 2, S * S
    out = [("empty", [], [], None), ("lone_centre", [P(c, c)], [], None)]
    if S >= 7:
        out.append(("lone_34", [2 * S + 3], [], None))
    if S >= 9:
        out.append(("lone_44", [P(3, 3)], [], None))
    out.append(("corners", [P(2, 2)], [P(S - 3, S - 3)], None) if S >= 7 else ("corners", [P(1, 1)], [P(3, 3)], None))
    out.append(("full", list(range(N)), [], None))
    out.append(("contact", [P(c, c), P(c, c + 1)], [P(c + 1, c)], None))
    out.append(("last_lines", [P(x, S - 1) for x in range(S - 1)], [P(S - 1, y) for y in range(S - 2)], None))
    out.append(("right_edge", [P(S - 1, 1)], [P(0, 3)], None))
    out.append(("walls", [P(x, 1) for x in range(S)], [P(x, S - 2) for x in range(S)], None))
    stray = [a for a in (N, N + 3, 32 * ((N + 31) // 32) - 1) if a >= N]
    out.append(("dead_inside", [P(x, 2) for x in range(S)] + [P(S - 2, S - 1)], [P(x, S - 2) for x in range(S)] + [P(1, 0)],
                sorted({P(1, 0), P(S - 2, S - 1), P(3, 0), P(S - 1, S - 1)} | set(stray))))
    out.append(("half_split", [P(x, y) for y in range(S) for x in range(c)], [P(x, y) for y in range(S) for x in range(c + 1, S)], None))
    return out


@functools.lru_cache(maxsize=None)
def case_points(S):
    """[(name, black, white, white to play, dead points or None)]"""
    out = []
    for name, b, w, dead in positions(S):
        out.append((name + "_sb", list(b), list(w), False, dead))
        out.append((name + "_cw", list(w), list(b), True, dead))
    return out


@functools.lru_cache(maxsize=None)
def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW], dead uint32 [n, NW]): the constructed positions over a random pattern.  A case without
    a `dead` set has a zero row."""
    rng = np.random.RandomState(5000 * S + seed)
    NW = (S * S + 31) // 32
    names, recs, dead = [], [], []
    for name, b, w, wtp, d in case_points(S):
        names.append(name)
        recs.append(build_record(S, b, w, wtp, rng))
        dead.append(M.words_of(d or [], NW))
    return names, np.stack(recs), np.stack(dead)


@functools.lru_cache(maxsize=None)
def case_model(S, triple, with_dead=True):
    """the model's outputs on case_records(S) at a parameter triple, computed once and shared (read only)"""
    _, recs, dead = case_records(S)
    return M.influence(S, recs, None, dead if with_dead else None, *triple)


@functools.lru_cache(maxsize=None)
def extra_records(S):
    """positions of play: the first rule shapes of the size, and at 19x19 every 64th position of the golden games"""
    shapes = rule_shape_records(S, 8)
    return np.concatenate([shapes, golden_records()[::16]]) if S == 19 else shapes


@functools.lru_cache(maxsize=None)
def extra_model(S, triple):
    return M.influence(S, extra_records(S), None, None, *triple)
