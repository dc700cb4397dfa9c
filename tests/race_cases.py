"""The case set of the capturing-race tests: constructed positions, each drawn at the smallest size at which it shows its point
(top-left corner; X black) and placed at every larger size too, for both sides to move over random words in planes 4..15 and in the
padding.  tests/test_race_model_power.py shows what each case reaches and which fault switch of tests/race_model.py it notices;
tests/test_gpu_race.py runs the same records on the device.

Every case names the two points it ASKS about (and, some, an explicit region); the same records are also ENUMERATED.
  tiny        the smallest race drawn here: three black stones with one liberty in the corner against two white stones with two
  box         a 3 x 3 box walled by a black and a white chain: a black and a white stone with three liberties each that touch only
              across the centre point; the black one gets more than max_libs = 3 liberties by extending to the centre
  run         a black stone in atari between two white stones on the edge: it saves itself by capturing the corner stone (an inner
              chain of M), and where it extends instead it reaches a liberty outside M
  ko          the ko of tests/solve_cases.py; the asked black stone is in atari, read in the one-point region of the ko point: with
              `prev` saying that white's stone vanished there, white to play may not retake at the root
  open        two stones far from everything: SGO_RACE_OPEN
  empty_point, point_n, negative, one_colour     SGO_RACE_NO_PAIR
  seki, eye   (7x7) the issue's table: two shared liberties and no eye / an eye against no eye
  nakade      (7x7) the black racer's only liberty is the point beside a white stone inside its eye: the inner-chain rule
  connect     (7x7) `connect` of tests/solve_cases.py read in the one-point region of the connecting point: it has no empty
              neighbour and captures nothing, so rules = 0 forbids it (caught) and rules = 1 plays it, and the joined chain has its
              liberties outside M (unsettled)
  plain_2v2, plain_2v1, shared    (9x9) the issue's table
  deep_case() (19x19 only, max_region 32) two one-eyed racers and a walled 6 x 5 block of empty points: the first line of play passes
              depth 80"""
import functools

import numpy as np

from tests import race_model as M
from tests.tactics_cases import diagram

SIZES = M.SIZES
MAX_LIBS, MAX_REGION, MAX_NODES = 3, 8, 4096
TABLE = {"plain_2v2": (["O.XXOO.X.", "O.XXOO.X.", "OOOOXXXX."], (2, 4)), "plain_2v1": (["O.XXOOXX.", "O.XXOO.X.", "OOOOXXXX."], (2, 4)),
         "shared": (["O.XX.OO.X", "OOXXXOOXX", ".OOOOXXX."], (2, 5)), "seki": (["OXX.OOX", "OXX.OOX", "OXXXOOX", "OOOOXXX"], (1, 4)),
         "eye": ([".XX.OOX", "XXX.OOX", "XXXXOOX", "OOOOXXX"], (1, 4))}

DEEP_LIBS, DEEP_REGION, DEEP_NODES = 8, 32, 600


@functools.lru_cache(maxsize=None)
def deep_case():
    """(record, asked pair, region words): 19x19.  The racers stand in the bottom-left corner, each with ONE one-point eye as its only
    liberty, walled off from everything else; the region is the two eyes and a 6 x 5 block of empty points in the top-left corner
    walled by a black chain.  Candidates ascend, so the first line of play fills and empties the block and never reaches the eyes:
    query A of the black racer ends unknown at the depth cap after 92 nodes; the white racer's queries spend the node budget"""
    S = 19
    P = lambda x, y: y * S + x                                                           # noqa: E731
    b, w = diagram(S, [".....X"] * 6 + ["XXXXXX"] + [""] * 9 + ["OOOOXXXXXX", "XXXXOOOOOX", ".XXXOOO.OX"])
    region = M._words([P(x, y) for y in range(6) for x in range(5)] + [P(0, 18), P(7, 18)], 12)
    return M.build_record(S, b, w, True, None, None, np.random.RandomState(19)), (P(0, 17), P(4, 17)), region


@functools.lru_cache(maxsize=None)
def deep_model(fault=None):
    rec, pq, region = deep_case()
    return M.race(19, rec[None], ask=[pq], region=region[None], rules=1, max_libs=DEEP_LIBS, max_region=DEEP_REGION, max_nodes=DEEP_NODES,
                  fault=fault)


@functools.lru_cache(maxsize=None)
def positions(S):
    """[(name, black, white, black one ply ago or None, white one ply ago or None, asked pair, explicit region points or None)]"""
    P = lambda x, y: y * S + x                                                           # noqa: E731
    out = []

    def add(name, rows, ask, region=None, pb=None, pw=None):
        b, w = diagram(S, rows)
        out.append((name, b, w, pb, pw, ask, region))

    add("tiny", [".XO", "XXO", "OOXX"], (P(2, 1), P(1, 1)))
    add("box", ["...X", "X.OX", "...X", "OOOX"], (P(0, 1), P(2, 1)))
    add("run", ["OXO"], (P(1, 0), P(2, 0)))
    b, w = diagram(S, [".XO", "X.XO", ".XO"])
    out.append(("ko", b, w, [a for a in b if a != P(2, 1)], sorted(w + [P(1, 1)]), (P(2, 1), P(2, 0)), [P(1, 1)]))
    add("open", ["", "", "..X.O"], (P(2, 2), P(4, 2)))
    add("empty_point", ["XO"], (P(1, 1), P(1, 0)))
    add("point_n", ["XO"], (P(0, 0), S * S))
    add("negative", ["XO"], (P(1, 0), -1))
    add("one_colour", ["XO", "X"], (P(0, 0), P(0, 1)))
    if S >= 7:
        add("seki", TABLE["seki"][0], (P(1, 0), P(4, 0)))
        add("eye", TABLE["eye"][0], (P(5, 1), P(2, 2)))
        add("nakade", ["O.XXO.X", "XXXXO.X", "OOOOXXX"], (P(2, 0), P(4, 0)))
        add("connect", [".X.X.XO", "XXXXOOO", "OOOOO"], (P(5, 0), P(6, 0)), [P(4, 0)])
    if S >= 9:
        for name in ("plain_2v2", "plain_2v1", "shared"):
            add(name, TABLE[name][0], TABLE[name][1])
    return out


@functools.lru_cache(maxsize=None)
def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW], ask int32 [n, 2], region uint32 [n, NW] with the whole board where a case gives none,
    has_region bool [n]): every constructed position for both sides to move over a random pattern"""
    rng = np.random.RandomState(9000 * S + seed)
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
def asked_model(S, rules, fault=None, max_nodes=MAX_NODES):
    """the model on case_records(S), every row asked in its default region"""
    names, recs, ask, region, has = case_records(S)
    return M.race(S, recs, ask=ask, rules=rules, max_libs=MAX_LIBS, max_region=MAX_REGION, max_nodes=max_nodes, fault=fault)


@functools.lru_cache(maxsize=None)
def region_model(S, rules, fault=None):
    """the model on the cases that give a region, asked in it: (the record numbers, the outputs)"""
    names, recs, ask, region, has = case_records(S)
    pick = np.flatnonzero(has)
    return pick, M.race(S, recs, index=pick, ask=ask[pick], region=region[pick], rules=rules, max_libs=MAX_LIBS, max_region=MAX_REGION,
                        max_nodes=MAX_NODES, fault=fault)


@functools.lru_cache(maxsize=None)
def enumerated_model(S, rules, fault=None, max_pairs=M.MAX_PAIRS):
    """the model on case_records(S), every row enumerated"""
    names, recs, ask, region, has = case_records(S)
    return M.race(S, recs, rules=rules, max_libs=MAX_LIBS, max_region=MAX_REGION, max_nodes=MAX_NODES, max_pairs=max_pairs, fault=fault)


GOLDEN_LIBS, GOLDEN_REGION, GOLDEN_NODES, GOLDEN_PAIRS = 4, 5, 128, 64


@functools.lru_cache(maxsize=None)
def golden_sample(S):
    """solve_cases.golden_sample(S) below 19x19; at 19x19 one position of the golden game records"""
    from tests import solve_cases
    from tests.tactics_cases import golden_records
    return golden_records()[30:31] if S == 19 else solve_cases.golden_sample(S)


@functools.lru_cache(maxsize=None)
def golden_model(S):
    return M.race(S, golden_sample(S), rules=1, max_libs=GOLDEN_LIBS, max_region=GOLDEN_REGION, max_nodes=GOLDEN_NODES, max_pairs=GOLDEN_PAIRS)
