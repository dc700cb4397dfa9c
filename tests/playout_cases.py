"""The case set of the light-playout tests: constructed records at every size, and the RUNS (rows, per_row, rules, max_plies,
seed) the tests make over them.  tests/test_playout_model_power.py shows that the runs notice every fault switch of
tests/playout_model.py; tests/test_gpu_playout.py makes the same runs on the device and compares word for word.

THE POSITIONS.  Every position is given for both colours (the second with black and white exchanged and the flag flipped, so half
of the records have white to move) over random words in planes 4..15 and in the padding.
  eye shapes in the top-left corner of an otherwise open board, the eye the mover's: an interior eye with 0, 1 and 2 opponent
    diagonals, an edge eye with 0 and 1, a corner eye with 0 and 1, a would-be eye with one opponent neighbour; at 5x5 the shapes
    reach the far edges.
  the SPLIT board: black holds the columns x <= 1 but its corner eyes (0,0), (0,S-1), white the columns x >= 2 but its corner eyes
    (S-1,0), (S-1,S-1): nobody has a candidate (two passes, ply 2, not capped).  Its prev planes equal its stones, as after a pass
    in the record's history.
  ko on the split board, points p = (1,2) and q = (2,2): `ko_ban` has black's stone on q, white to move and white's stone on p
    in the history plane, so the root forbids the retake and white passes; `ko_free` is the same with a quiet history: white
    retakes, which bans black inside the playout, black passes and the pass lifts the ban; `connect` is ko_ban's stones with
    BLACK to move: p has no empty neighbour and captures nothing, so it is a candidate under rules = 1 alone.
    With the two-point hole (3,3), (3,4) in white's wall (`ko_hole`) both sides have a move elsewhere while the ko stands.
  a FULL board (no liberty anywhere: an illegal record), the full board with one hole, the EMPTY board.
  `words`: stones on both sides of every 32-bit word boundary of the planes (a = 32k - 1 black, 32k white).
THE RUNS.  `short`: every position, three playouts, six plies, both rule sets.  `end`: the split-board family to the end, four
playouts per row.  `counts`: per_row 1, 2, 3, one unit, one unit plus one under max_plies = 1 (every playout
capped after one ply).  `games`: whole games from the empty board and from the eye shapes, as many as the size affords the model."""
import functools

import numpy as np

from tests import playout_model as PM
from tests.tactics_cases import diagram

SIZES = PM.SIZES
UNIT = 16                                                            # csrc/sgo_playout.hip PLAYOUT_UNIT
GAMES = {5: 33, 7: 17, 9: 17, 13: 4, 19: 2}
END_PER_ROW = 4


def _split(S):
    P = lambda x, y: y * S + x                                                           # noqa: E731
    black = [P(x, y) for y in range(S) for x in (0, 1) if (x, y) not in ((0, 0), (0, S - 1))]
    white = [P(x, y) for y in range(S) for x in range(2, S) if (x, y) not in ((S - 1, 0), (S - 1, S - 1))]
    return black, white


def positions(S):
    """[(name, black, white, white_to_play, black one ply ago or None, white one ply ago or None)]"""
    N = S * S
    P = lambda x, y: y * S + x                                                           # noqa: E731
    out = []
    shapes = {
        "eye_in0": [".....", "..X..", ".X.X.", "..X.."],
        "eye_in1": [".....", ".OX..", ".X.X.", "..X.."],
        "eye_in2": [".....", ".OX..", ".X.X.", "..XO."],
        "eye_edge0": [".X.X.", "..X.."],
        "eye_edge1": [".X.X.", ".OX.."],
        "eye_corner0": [".X...", "X...."],
        "eye_corner1": [".X...", "XO..."],
        "eye_not": [".....", "..X..", ".X.X.", "..O.."],
        "eye_far": [".....", ".....", "...X.", "..X.X", "...X."],
    }
    for name, rows in shapes.items():
        b, w = diagram(S, rows)
        out.append((name, b, w, False, None, None))
    b, w = _split(S)
    p, q = P(1, 2), P(2, 2)
    out.append(("none", b, w, False, None, None))
    kb, kw = sorted(set(b) - {p} | {q}), sorted(set(w) - {q})
    out.append(("ko_ban", kb, kw, True, sorted(set(kb) - {q}), sorted(set(kw) | {p})))
    out.append(("ko_free", kb, kw, True, None, None))
    out.append(("connect", kb, kw, False, None, None))
    hole = {P(3, 3), P(3, 4)} if S > 5 else {P(3, 3), P(4, 3)}
    out.append(("ko_hole", kb, sorted(set(kw) - hole), True, None, None))
    out.append(("ko_hole_b", kb, sorted(set(kw) - hole), False, None, None))
    full_b = [P(x, y) for y in range(S) for x in range(S) if x < S // 2]
    full_w = [a for a in range(N) if a not in set(full_b)]
    out.append(("full", full_b, full_w, False, None, None))
    out.append(("full_but_one", sorted(set(full_b) - {P(S // 2 - 1, 1)}), full_w, False, None, None))
    out.append(("full_but_two", sorted(set(full_b) - {P(S // 2 - 1, 1)}), sorted(set(full_w) - {P(S - 1, S - 1)}), False, None, None))
    out.append(("empty", [], [], False, None, None))
    out.append(("words", [a for a in range(31, N, 32)], [a for a in range(32, N, 32)], False, None, None))
    return out


@functools.lru_cache(maxsize=None)
def case_records(S):
    """(names, records uint32 [R, 16 * NW]): every position, then every position with the colours exchanged"""
    rng = np.random.RandomState(8000 * S)
    names, recs = [], []
    for swap in (False, True):
        for name, b, w, wtp, pb, pw in positions(S):
            if swap:
                b, w, wtp, pb, pw = w, b, not wtp, pw, pb
            names.append(name + ("_x" if swap else ""))
            recs.append(PM.build_record(S, b, w, wtp, pb, pw, rng))
    return tuple(names), np.stack(recs)


def _rows(S, *wanted):
    names = case_records(S)[0]
    return [i for i, nm in enumerate(names) if nm[:-2] in wanted or nm in wanted]


@functools.lru_cache(maxsize=None)
def runs(S):
    """[(name, index or None, per_row, rules, max_plies, seed)]"""
    out = []
    for rules in (0, 1):
        out.append(("short_r%d" % rules, None, 3, rules, 6, 11))
        out.append(("end_r%d" % rules, tuple(_rows(S, "none", "ko_ban", "ko_free", "connect", "ko_hole", "ko_hole_b", "full", "full_but_one",
                                                      "full_but_two")), END_PER_ROW, rules, 0, 12))
    for per_row in (1, 2, 3, UNIT, UNIT + 1):
        out.append(("counts_%d" % per_row, tuple(_rows(S, "empty", "ko_free", "eye_in2")), per_row, 1, 1, 13))
    g = GAMES[S]
    start = ("empty",) if S > 9 else ("empty", "eye_in0", "eye_edge1", "eye_corner0")
    out.append(("games_r1", tuple(_rows(S, *start)), g, 1, 0, 14))
    if S <= 13:
        out.append(("games_r0", tuple(_rows(S, *start)), g, 0, 0, 15))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def run_model(S, name, fault=None):
    """the model's outputs of one run, computed once and shared (read only)"""
    recs = case_records(S)[1]
    for nm, index, per_row, rules, max_plies, seed in runs(S):
        if nm == name:
            return PM.playouts(S, recs, index, per_row, seed, rules, max_plies, fault)
    raise KeyError(name)


GOLDEN_PER_ROW, GOLDEN_SEED = 1, 16


@functools.lru_cache(maxsize=None)
def golden_records():
    """every 16th position of the five golden 19x19 games"""
    from tests.tactics_cases import golden_records as every
    return every(16)


@functools.lru_cache(maxsize=None)
def golden_model():
    return PM.playouts(19, golden_records(), None, GOLDEN_PER_ROW, GOLDEN_SEED, 1, 0)
