"""The case set of the chains-and-ladders tests: constructed positions at the smallest sizes at which each can go wrong, for both
sides to move over random words in planes 4..15 and in the padding, then the positions of rule_shapes_S*.npz and every fourth
position of the golden 19x19 records (replayed by the records model).  tests/test_tactics_model_power.py shows what each case
reaches and which fault switch of tests/tactics_model.py it notices; tests/test_gpu_tactics.py runs the same records on the device.

THE CAPS.  No position was found whose query ends exactly at 512 nodes with a neighbour at 513: the node count of a query is the
size of a whole search tree, and one stone more changes it by dozens.  The node cap is reached at its real value by what crosses
it: golden positions hold queries that end unknown at 513 nodes (test_tactics_model_power.py counts them).  The depth cap is
crossed by `ladder_deep` (19x19), a ladder that a few stones near the far corner bend back: its query A reaches depth 81 after 126
nodes and ends unknown there.  Its neighbour below the cap is golden position 260, where a query visits nodes at depth 80, not
beyond, and goes on (to the node cap): a reader that gave up at depth 80 would stop it early.  A straight ladder across the whole
board (`ladder`) is 59 plies deep."""
import functools

import numpy as np

from tests import tactics_model as T

SIZES = T.SIZES
# found by a random search over ladders with a few extra stones near the far corner (the model decided)
DEEP_BLACK, DEEP_WHITE = [(10, 17), (13, 18)], [(14, 14), (18, 18), (12, 15), (13, 17), (10, 16)]


def diagram(S, rows, ox=0, oy=0):
    """(black, white) point lists of an ASCII picture (X black, O white) with its top-left corner at (ox, oy)"""
    black, white = [], []
    for y, line in enumerate(rows):
        for x, ch in enumerate(line.replace(" ", "")):
            if ch in "XO":
                (black if ch == "X" else white).append((oy + y) * S + ox + x)
    return sorted(black), sorted(white)


def ladder(S, extra_black=(), extra_white=()):
    """black on the 4-4 point with two liberties, white's three stones that make the ladder run down-right to the edge"""
    P = lambda x, y: y * S + x                                                           # noqa: E731
    return sorted([P(3, 3)] + [P(x, y) for x, y in extra_black]), sorted([P(3, 2), P(2, 3), P(4, 2)] + [P(x, y) for x, y in extra_white])


def lattice(S):
    """Single stones in a checkerboard of colours with every fifth point empty ((x + 2y) % 5 == 0: every point has exactly one
    such point among itself and its neighbours), chains without a liberty at the edge taken off: hundreds of chains in atari."""
    stones = {}
    for y in range(S):
        for x in range(S):
            if (x + 2 * y) % 5:
                stones[y * S + x] = 1 if (x + y) % 2 else -1
    while True:
        bad = [a for a in stones if not any(0 <= a % S + dx < S and 0 <= a // S + dy < S and (a + dy * S + dx) not in stones
                                            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)))]
        if not bad:
            break
        for a in bad:
            del stones[a]
    return sorted(a for a, c in stones.items() if c == 1), sorted(a for a, c in stones.items() if c == -1)


@functools.lru_cache(maxsize=None)
def positions(S):
    """[(name, black, white, black one ply ago or None, white one ply ago or None)]"""
    P = lambda x, y: y * S + x                                                           # noqa: E731
    out = [("empty", [], [], None, None)]
    # a chain saved only by a counter-capture: black (0,0) is in atari, extending dies, taking white (1,0) lives
    b, w = diagram(S, ["XOX", ".", "O"])
    out.append(("counter_capture", b, w, None, None))
    # the ko: black has just taken at (2,1); white may not retake at (1,1) when it is white's turn -- and may in a query whose
    # root mover is not the side to move.  With black to move, white's capture at (1,1) inside the tree makes black's retake the ko.
    b, w = diagram(S, [".XO", "X.XO", ".XO"])
    out.append(("ko", b, w, [a for a in b if a != P(2, 1)], sorted(w + [P(1, 1)])))
    # the attacker's move into the eye is suicide (not allowed); the outside liberty catches the chain
    b, w = diagram(S, [".XO", "XXO", "O."])
    out.append(("suicide", b, w, None, None))
    if S >= 7:
        # snapback: white's throw-in at (2,2) is captured by (3,2), which leaves the chain with one liberty
        b, w = diagram(S, [".OOO.", "OXXXO", "OX..O", "OXXXO", ".OOO."])
        out.append(("snapback", b, w, None, None))
    if S >= 9:
        b, w = ladder(S)
        out.append(("ladder", b, w, None, None))
        b, w = ladder(S, extra_black=[(S - 3, S - 3)])
        out.append(("ladder_breaker", b, w, None, None))
        b, w = ladder(S, extra_white=[(S - 3, S - 3)])
        out.append(("ladder_into_attacker", b, w, None, None))
        b, w = ladder(S, extra_white=[(3, 4)])                       # in atari: caught even with the defender first
        out.append(("ladder_atari", b, w, None, None))
        # the ladder's chain row next to short queries in the same wavefront: a stone in atari in the far corner, a lone stone
        b, w = ladder(S, extra_black=[(0, 0), (S - 1, 0)], extra_white=[(S - 1, 1)])
        out.append(("ladder_beside", b, w, None, None))
    if S == 19:
        b, w = lattice(S)
        out.append(("lattice", b, w, None, None))
        # a ladder that stones near the far corner bend back: query A passes depth 80 and ends unknown at the depth cap
        b, w = ladder(S, extra_black=DEEP_BLACK, extra_white=DEEP_WHITE)
        out.append(("ladder_deep", b, w, None, None))
    return out


def rule_shape_records(S, limit=24):
    from tests import rollout_model as rm
    from tests.rule_shapes import load_shapes
    return rm.pack_boards(load_shapes(S).boards[:limit])


@functools.lru_cache(maxsize=None)
def golden_records(every=4):
    """every fourth record of the five golden 19x19 games, replayed by the records model (history planes as the games made them)"""
    from tests import records_model as M
    from tests.helpers import load
    z = load("sgf_S19.npz")
    S = int(z["size"])
    games = []
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        games.append(([S * S if y >= S else int(y) * S + int(x) for x, y, _ in mv], [int(c) for _, _, c in mv]))
    return M.replay(S, games)["records"][::every].copy()


@functools.lru_cache(maxsize=None)
def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW]): every constructed position for both sides to move over a random pattern, then the
    rule shapes"""
    rng = np.random.RandomState(2000 * S + seed)
    names, recs = [], []
    for name, b, w, pb, pw in positions(S):
        for wtp in (False, True):
            names.append("%s_%s" % (name, "w" if wtp else "b"))
            recs.append(T.build_record(S, b, w, wtp, pb, pw, rng))
    shapes = rule_shape_records(S)
    names += ["shape_%d" % i for i in range(len(shapes))]
    return names, np.concatenate([np.stack(recs), shapes])


@functools.lru_cache(maxsize=None)
def case_model(S):
    """the model's outputs on case_records(S), computed once and shared (read only)"""
    names, recs = case_records(S)
    return T.tactics(S, recs)


@functools.lru_cache(maxsize=None)
def golden_model():
    return T.tactics(19, golden_records())
