"""The case set of the move-outcome tests: constructed positions drawn into the top-left corner, so that the whole set stands at 5x5
and again at every larger size, each for both colours to move over random words in planes 4..15 and in the padding; then the
positions of rule_shapes_S*.npz; at 19x19 one chain that runs over the rows straddling the 32-bit word boundaries of the packed
plane.  tests/test_moves_model_power.py shows which fault switch of tests/moves_model.py each case notices;
tests/test_gpu_moves.py runs the same records on the device."""
import functools

import numpy as np

from tests import moves_model as M
from tests.tactics_cases import diagram, golden_records, rule_shape_records  # noqa: F401
from tests.tactics_model import build_record

SIZES = M.SIZES


@functools.lru_cache(maxsize=None)
def positions(S):
    """[(name, black, white, black one ply ago or None, white one ply ago or None)]"""
    P = lambda x, y: y * S + x                                                           # noqa: E731
    out = [("empty", [], [], None, None)]                            # corner and edge quiet points: 2 and 3 liberties
    # the ko: black has just taken at (2,1); white may not retake at (1,1) -- which would capture and is allowed otherwise
    b, w = diagram(S, [".XO", "X.XO", ".XO"])
    out.append(("ko", b, w, [a for a in b if a != P(2, 1)], sorted(w + [P(1, 1)])))
    # the same stones, but two of white's stones are gone since the last ply: not a ko
    out.append(("ko_two_gone", b, w, [a for a in b if a != P(2, 1)], sorted(w + [P(1, 1), P(0, 0)])))
    # snapback: white takes the stone on (0,0) with (1,0) and stands with five stones on one liberty, the point just emptied;
    # black on (1,0) takes four.  The merged chain's only liberty is a captured point.
    b, w = diagram(S, ["X.OX", "OOOX", "XXXX"])
    out.append(("snapback", b, w, None, None))
    # black (1,0) joins (0,0) into two stones without a liberty and captures nothing: a two-stone suicide
    b, w = diagram(S, ["X.O", "OO"])
    out.append(("suicide2", b, w, None, None))
    # black (1,0) has no empty neighbour and is allowed only because it captures -- two chains at once; two more white stones in
    # atari stand far from it in the opposite corner, so two points capture two stones each
    b, w = diagram(S, ["O.OX", "XXX"])
    b, w = sorted(b + [P(S - 3, S - 1), P(S - 2, S - 2)]), sorted(w + [P(S - 2, S - 1), P(S - 1, S - 1)])
    out.append(("two_chains", b, w, None, None))
    # (2,2) joins four black chains; the left one has only that liberty
    b, w = diagram(S, ["..X", ".OX", "OX.X", ".OX"])
    out.append(("join4", b, w, None, None))
    # (0,0) has no empty neighbour, joins a black chain with liberties and captures nothing: forbidden, but sound
    b, w = diagram(S, [".X", "XX"])
    out.append(("forbidden_sound", b, w, None, None))
    # one black chain touches (2,2) twice; with white's stones around it a white stone there leaves it one liberty
    b, w = diagram(S, [".OO", "OXXO", "OX"])
    out.append(("twice", b, w, None, None))
    # every point but the centre holds a black stone
    c = P(S // 2, S // 2)
    out.append(("full_minus_one", [a for a in range(S * S) if a != c], [], None, None))
    if S == 19:
        # a black chain down column 13 and along row 1 (bits 29..35: over the first word boundary; 127 / 128: the fourth), white
        # stones against it on both sides of a boundary
        b = sorted({P(13, y) for y in range(0, 9)} | {P(x, 1) for x in range(10, 17)})
        w = sorted([P(12, 2), P(14, 2), P(12, 6), P(14, 6), P(9, 1), P(17, 1), P(13, 9)])
        out.append(("straddle", b, w, None, None))
    return out


@functools.lru_cache(maxsize=None)
def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW]): every constructed position for both colours to move over a random pattern, then the
    rule shapes"""
    rng = np.random.RandomState(3000 * S + seed)
    names, recs = [], []
    for name, b, w, pb, pw in positions(S):
        for wtp in (False, True):
            names.append("%s_%s" % (name, "w" if wtp else "b"))
            recs.append(build_record(S, b, w, wtp, pb, pw, rng))
    shapes = rule_shape_records(S)
    names += ["shape_%d" % i for i in range(len(shapes))]
    return names, np.concatenate([np.stack(recs), shapes])


def contact_points(S, rec):
    """the number of empty points of a record next to a stone: the trips of the kernel's candidate loop for it"""
    board = M.read_record(S, rec)[0]
    nbrs = M.neighbours(S, S * S)
    return sum(1 for a in range(S * S) if board[a] == M.EMPTY and any(board[q] != M.EMPTY for q in nbrs[a]))


@functools.lru_cache(maxsize=None)
def case_model(S, side):
    """the model's outputs on case_records(S), computed once and shared (read only)"""
    return M.moves(S, case_records(S)[1], side=side)


# the stride of test_gpu_moves.test_golden_positions over tactics_cases.golden_records(every=1), all records of the five golden
# 19x19 games: every 32nd record and each game's last
GOLDEN_STRIDE = 32


@functools.lru_cache(maxsize=None)
def golden_sample():
    """(records, model side 0, model side 1) of the golden positions the device test compares"""
    from tests.helpers import load
    g = golden_records(1)
    z = load("sgf_S19.npz")
    keep, end = set(range(0, len(g), GOLDEN_STRIDE)), 0
    for gi in range(5):
        end += len(z["g%02d_moves" % gi]) + 1
        keep.add(end - 1)
    assert end == len(g)
    recs = g[sorted(keep)].copy()
    return recs, M.moves(19, recs, side=0), M.moves(19, recs, side=1)


def golden_sample_index():
    """the indices of golden_sample()'s records in tactics_cases.golden_records(1)"""
    from tests.helpers import load
    z = load("sgf_S19.npz")
    ends = np.cumsum([len(z["g%02d_moves" % gi]) + 1 for gi in range(5)])
    return sorted(set(range(0, int(ends[-1]), GOLDEN_STRIDE)) | {int(e) - 1 for e in ends})
