"""The case set of the life-and-death tests: constructed positions, each drawn at the smallest size at which it shows its point
(top-left corner; X black is the colour the pictures are about) and placed at every larger size too, for both sides to move over
random words in planes 4..15 and in the padding.  tests/test_solve_model_power.py shows what each case reaches and which fault
switch of tests/solve_model.py it notices; tests/test_gpu_solve.py runs the same records on the device.

Every case names the point it ASKS about (and, some, an explicit region); the same records are also ENUMERATED.
  two_eyes        two one-point eyes: alive at the root, nodes 1; asked through a stone that is not the anchor
  straight_three  three points in a row on the edge
  bulky_five      the five-point eye whose vital point is (1, 0)
  straight_four   four points in a row on the edge
  square_four     the 2x2 eye in the corner
  seki            X and an inner O chain of three share two liberties (what either side captures there is a living four-point eye),
                  and X has one more liberty outside: X lives only by passing
  nakade          X and an inner O chain with an eye each share one liberty: the kill captures and replays inside the eye
  ko              the ko of tests/tactics_cases.py; the asked stone is the one in atari, read in the one-point region of the ko
                  point: with `prev` saying that white's stone vanished there, white to play may not retake at the root
  connect         a stone in atari beside a two-eyed group; the connecting point has no empty neighbour and captures nothing, so
                  rules = 0 forbids it (DEAD) and rules = 1 plays it (unsettled)
  connect_small   the same, asked with an explicit region that leaves the connecting point out: nobody can play there
  open            a lone stone on the open board: SGO_SOLVE_OPEN
  no_stone        an asked empty point; `outside` asks the point N
  deep_case()     (19x19 only, max_region 32) a 3 x 10 block of empty points whose first line of play passes depth 80: the depth cap

THE WAIT.  straight_three, bulky_five and square_four are killed through a capture of ONE stone inside the last eye and the replay
on that point, which the one-stone ko approximation forbids for a ply; the attacker's WAIT (while such a ban is in force) is what
reads them as a player does, and the `no_wait` switch of the model reads all three alive."""
import functools

import numpy as np

from tests import solve_model as M
from tests.tactics_cases import diagram

SIZES = M.SIZES
MAX_REGION, MAX_NODES = 6, 4096


DEEP_REGION, DEEP_NODES = 32, 600


@functools.lru_cache(maxsize=None)
def deep_case():
    """(record, asked point): 19x19, a chain around a 3 x 10 block of empty points in the corner.  The first line of play of
    query A fills and empties the block for 80 plies and goes on: the query ends unknown at the depth cap after 336 nodes"""
    S = 19
    b, w = diagram(S, ["." * 10 + "XO", "." * 10 + "XO", "." * 10 + "XO", "X" * 11 + "O", "O" * 12])
    return M.build_record(S, b, w, True, None, None, np.random.RandomState(19)), 10


@functools.lru_cache(maxsize=None)
def deep_model(fault=None):
    rec, a = deep_case()
    return M.solve(19, rec[None], ask=[a], rules=1, max_region=DEEP_REGION, max_nodes=DEEP_NODES, fault=fault)


@functools.lru_cache(maxsize=None)
def positions(S):
    """[(name, black, white, black one ply ago or None, white one ply ago or None, asked point, explicit region points or None)]"""
    P = lambda x, y: y * S + x                                                           # noqa: E731
    out = []

    def add(name, rows, ask, region=None, pb=None, pw=None):
        b, w = diagram(S, rows)
        out.append((name, b, w, pb, pw, ask, region))

    add("two_eyes", [".X.XO", "XXXXO", "OOOOO"], P(3, 1))
    add("straight_three", ["...XO", "XXXXO", "OOOOO"], P(3, 0))
    add("square_four", ["..XO", "..XO", "XXXO", "OOOO"], P(2, 0))
    b, w = diagram(S, [".XO", "X.XO", ".XO"])
    out.append(("ko", b, w, [a for a in b if a != P(2, 1)], sorted(w + [P(1, 1)]), P(2, 1), [P(1, 1)]))
    add("open", ["", "", "..X"], P(2, 2))
    add("no_stone", ["X"], P(1, 1))
    add("outside", ["X"], S * S)
    if S >= 7:
        add("bulky_five", ["...XO", "..XXO", "XXXOO", "OOOO"], P(3, 0))
        add("straight_four", ["....XO", "XXXXXO", "OOOOOO"], P(4, 0))
        add("seki", ["OOO.XO", "XX.XXO", "XXXXOO", ".OOOO", "OO"], P(4, 0))
        add("nakade", [".O.X.XO", "OOXXXXO", "XXXOOOO", "OOOO"], P(3, 0))
        add("connect", [".X.X.XO", "XXXXOOO", "OOOOO"], P(5, 0))
        add("connect_small", [".X.X.XO", "XXXXOOO", "OOOOO"], P(5, 0), [P(0, 0), P(2, 0)])
    return out


@functools.lru_cache(maxsize=None)
def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW], ask int32 [n], region uint32 [n, NW] with the whole board where a case gives none,
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
    return names, np.stack(recs), np.array(ask, np.int32), np.stack(region), np.array(has)


@functools.lru_cache(maxsize=None)
def asked_model(S, rules, fault=None, max_nodes=MAX_NODES):
    """the model on case_records(S), every row asked in its default region"""
    names, recs, ask, region, has = case_records(S)
    return M.solve(S, recs, ask=ask, rules=rules, max_region=MAX_REGION, max_nodes=max_nodes, fault=fault)


@functools.lru_cache(maxsize=None)
def region_model(S, rules, fault=None):
    """the model on the cases that give a region, asked in it: (the record numbers, the outputs)"""
    names, recs, ask, region, has = case_records(S)
    pick = np.flatnonzero(has)
    return pick, M.solve(S, recs, index=pick, ask=ask[pick], region=region[pick], rules=rules, max_region=MAX_REGION, max_nodes=MAX_NODES,
                         fault=fault)


@functools.lru_cache(maxsize=None)
def enumerated_model(S, rules, fault=None, max_targets=M.MAX_TARGETS):
    """the model on case_records(S), every row enumerated"""
    names, recs, ask, region, has = case_records(S)
    return M.solve(S, recs, rules=rules, max_region=MAX_REGION, max_nodes=MAX_NODES, max_targets=max_targets, fault=fault)


GOLDEN_REGION, GOLDEN_NODES, GOLDEN_TARGETS = 5, 256, 8


@functools.lru_cache(maxsize=None)
def golden_sample(S):
    """about ten plies spread over the games of tests/golden/rules_S<S>.npz (the last ply among them) and, at 19x19, one position
    of the golden game records (tactics_cases.golden_records()[30], a middle game with dozens of chains)"""
    from tests import rollout_model as rm
    from tests.helpers import load
    from tests.tactics_cases import golden_records
    zf = load("rules_S%d.npz" % S)
    boards = np.concatenate([zf["g%02d_fulls" % g].astype(np.int32) for g in range(int(zf["n_games"]))])
    k = max(1, len(boards) // 10)
    recs = rm.pack_boards(boards[k - 1::k])
    return np.concatenate([recs, golden_records()[30:31]]) if S == 19 else recs


@functools.lru_cache(maxsize=None)
def golden_model(S):
    return M.solve(S, golden_sample(S), rules=1, max_region=GOLDEN_REGION, max_nodes=GOLDEN_NODES, max_targets=GOLDEN_TARGETS)


def verdict(row):
    """`alive` / `unsettled` / `dead` / `unknown` / `open` / `no_stone` of a table row, as the header's status bits say"""
    st = int(row[3])
    if st & M.NO_STONE:
        return "no_stone"
    if st & M.OPEN:
        return "open"
    if st & (M.A_UNKNOWN | M.D_UNKNOWN):
        return "unknown"
    if not st & M.A_DEAD:
        return "alive"
    return "dead" if st & M.D_DEAD else "unsettled"
