"""The case set of the connection tests: constructed positions, each drawn at the smallest size at which it shows its point
(top-left corner; X black) and placed at every larger size too, for both sides to move over random words in planes 4..15 and in the
padding.  tests/test_connect_model_power.py shows what each case reaches and which fault switch of tests/connect_model.py it notices;
tests/test_gpu_connect.py runs the same records on the device.

Every case names the two points it ASKS about (and, some, an explicit region); the same records are also ENUMERATED.
  diagonal, bamboo, tiger_corner, jump, jump_edge, peep, cutter_atari, false_join, crosscut      the textbook shapes
  ko            two black chains whose only link point is a ko point white has just been captured on: white to play may not retake at
                the root, so it can only pass and black joins; with black to play in the record white's root move is free
  fill          the joining point has three black neighbours and no empty one and captures nothing: rules = 0 forbids it (cut),
                rules = 1 plays it (connected)
  diagonal_rev  the diagonal asked with the higher anchor first: the row is the diagonal's
  knight        a knight's move: no common liberty, four link points, `open` at max_region 8
  chain3        three black stones on a diagonal: the two neighbouring pairs are NEAR, the outer pair is not
  side3         the same with one-point jumps on the first line: both pairs connected, the outer pair not NEAR
  two_colours   a diagonal of each colour on one board: the group map holds both
  stones_far    two stones far from everything: not NEAR, SGO_CONNECT_OPEN when asked
  empty_point, point_n, negative, two_colour_ask, one_chain     SGO_CONNECT_NO_PAIR
  deep_case()   (19x19 only, max_region 32) a one-point jump on the first line read in a region that also holds a walled 6 x 5 block
                of empty points: the first line of play fills and empties the block and passes depth 80"""
import functools

import numpy as np

from tests import connect_model as M
from tests.tactics_cases import diagram

SIZES = M.SIZES
CUT_LIBS, MAX_REGION, MAX_NODES = 1, 8, 4096
# the issue's table: name -> (diagram, asked pair (x, y) (x, y), verdict, nodes of A, nodes of D or None)
TABLE = {"diagonal": (["", ".X...", "..X.."], ((1, 1), (2, 2)), "connected", 145, None),
         "bamboo": (["", ".XX..", ".....", ".XX.."], ((1, 1), (1, 3)), "connected", 49, None),
         "tiger_corner": ([".X.", "X.."], ((1, 0), (0, 1)), "connected", 9, None),
         "jump": (["", "", ".X.X."], ((1, 2), (3, 2)), "unsettled", 8, 10),
         "jump_edge": ([".X.X."], ((1, 0), (3, 0)), "connected", 9, None),
         "peep": (["", ".XO..", "..X.."], ((1, 1), (2, 2)), "unsettled", 8, 10),
         "cutter_atari": (["", ".XOX.", ".OX.."], ((1, 1), (3, 1)), "unsettled", 14, 20),
         "false_join": (["OX.XO", "OOXOO", ".O.O."], ((1, 0), (3, 0)), "unsettled", 1, 2),
         "crosscut": (["", ".XO..", ".OX.."], ((1, 1), (2, 2)), "open", None, None)}

DEEP_REGION, DEEP_NODES = 32, 600


@functools.lru_cache(maxsize=None)
def deep_case():
    """(record, asked pair, region words): 19x19.  A black one-point jump on the bottom line; the region is its link point and a 6 x 5
    block of empty points in the top-left corner walled by a black chain.  Candidates ascend, so the first line of play fills and
    empties the block and never reaches the link point: query A ends unknown at the depth cap"""
    S = 19
    P = lambda x, y: y * S + x                                                           # noqa: E731
    b, w = diagram(S, [".....X"] * 6 + ["XXXXXX"] + [""] * 11 + ["...X.X"])
    region = M._words([P(x, y) for y in range(6) for x in range(5)] + [P(4, 18)], 12)
    return M.build_record(S, b, w, True, None, None, np.random.RandomState(19)), (P(3, 18), P(5, 18)), region


@functools.lru_cache(maxsize=None)
def deep_model(fault=None):
    rec, pq, region = deep_case()
    return M.connect(19, rec[None], ask=[pq], region=region[None], rules=1, max_region=DEEP_REGION, max_nodes=DEEP_NODES, fault=fault)


@functools.lru_cache(maxsize=None)
def positions(S):
    """[(name, black, white, black one ply ago or None, white one ply ago or None, asked pair, explicit region points or None)]"""
    P = lambda x, y: y * S + x                                                           # noqa: E731
    out = []

    def add(name, rows, ask, region=None, pb=None, pw=None):
        b, w = diagram(S, rows)
        out.append((name, b, w, pb, pw, ask, region))

    for name, (rows, (p, q), _, _, _) in TABLE.items():
        add(name, rows, (P(*p), P(*q)))
    b, w = diagram(S, [".XO", "X.XO", ".XO"])
    out.append(("ko", b, w, [a for a in b if a != P(2, 1)], sorted(w + [P(1, 1)]), (P(1, 0), P(2, 1)), [P(1, 1)]))
    add("fill", ["X.X", ".X"], (P(0, 0), P(2, 0)))
    add("diagonal_rev", TABLE["diagonal"][0], (P(2, 2), P(1, 1)))
    add("knight", ["", ".X", "", "..X"], (P(1, 1), P(2, 3)))
    add("chain3", ["", ".X", "..X", "...X"], (P(1, 1), P(3, 3)))
    add("side3", ["X.X.X"], (P(0, 0), P(4, 0)))
    add("two_colours", ["X..O", ".XO"], (P(0, 0), P(1, 1)))
    add("stones_far", ["X", "", "", "", "....X"], (P(0, 0), P(4, 4)))
    add("empty_point", ["X.X"], (P(1, 1), P(0, 0)))
    add("point_n", ["X.X"], (P(0, 0), S * S))
    add("negative", ["X.X"], (P(2, 0), -1))
    add("two_colour_ask", ["X.O"], (P(0, 0), P(2, 0)))
    add("one_chain", ["XX"], (P(0, 0), P(1, 0)))
    return out


@functools.lru_cache(maxsize=None)
def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW], ask int32 [n, 2], region uint32 [n, NW] with the whole board where a case gives none,
    has_region bool [n]): every constructed position for both sides to move over a random pattern"""
    rng = np.random.RandomState(7000 * S + seed)
    NW = (S * S + 31) // 32
    names, recs, ask, region, has = [], [], [], [], []
    for name, b, w, pb, pw, a, reg in positions(S):
        for wtp in (False, True):
            names.append("%s_%s" % (name, "w" if wtp else "b"))
            recs.append(M.build_record(S, b, w, wtp, pb, pw, rng))
            ask.append(a)
            region.append(M._words(range(S * S) if reg is None else reg, NW))
            has.append(reg is not None)
    return names, np.stack(recs), np.array(ask, np.int32).reshape(-1, 2), np.stack(region), np.array(has)


@functools.lru_cache(maxsize=None)
def asked_model(S, rules, fault=None, max_nodes=MAX_NODES, cut_libs=CUT_LIBS):
    """the model on case_records(S), every row asked in its default region"""
    names, recs, ask, region, has = case_records(S)
    return M.connect(S, recs, ask=ask, rules=rules, cut_libs=cut_libs, max_region=MAX_REGION, max_nodes=max_nodes, fault=fault)


@functools.lru_cache(maxsize=None)
def region_model(S, rules, fault=None):
    """the model on the cases that give a region, asked in it: (the record numbers, the outputs)"""
    names, recs, ask, region, has = case_records(S)
    pick = np.flatnonzero(has)
    return pick, M.connect(S, recs, index=pick, ask=ask[pick], region=region[pick], rules=rules, cut_libs=CUT_LIBS, max_region=MAX_REGION,
                           max_nodes=MAX_NODES, fault=fault)


@functools.lru_cache(maxsize=None)
def enumerated_model(S, rules, fault=None, max_pairs=M.MAX_PAIRS, cut_libs=CUT_LIBS):
    """the model on case_records(S), every row enumerated"""
    names, recs, ask, region, has = case_records(S)
    return M.connect(S, recs, rules=rules, cut_libs=cut_libs, max_region=MAX_REGION, max_nodes=MAX_NODES, max_pairs=max_pairs, fault=fault)


GOLDEN_CUT_LIBS, GOLDEN_REGION, GOLDEN_NODES, GOLDEN_PAIRS = 1, 5, 128, 64


@functools.lru_cache(maxsize=None)
def golden_sample(S):
    """solve_cases.golden_sample(S) below 19x19; at 19x19 one position of the golden game records"""
    from tests import solve_cases
    from tests.tactics_cases import golden_records
    return golden_records()[30:31] if S == 19 else solve_cases.golden_sample(S)


@functools.lru_cache(maxsize=None)
def golden_model(S):
    return M.connect(S, golden_sample(S), rules=1, cut_libs=GOLDEN_CUT_LIBS, max_region=GOLDEN_REGION, max_nodes=GOLDEN_NODES,
                     max_pairs=GOLDEN_PAIRS)
