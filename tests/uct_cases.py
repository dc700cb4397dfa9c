"""The case set of the playout-tree-search tests: the records of tests/playout_cases.py plus one constructed here, and the RUNS the
tests make over them.  tests/test_uct_model_power.py shows that the runs notice every fault switch of tests/uct_model.py;
tests/test_gpu_uct.py makes the same runs on the device and compares word for word, the trace included.

THE EXTRA POSITION.  `two_kos`: the split board of tests/playout_cases.py with a ko in row 2 (black's stone on (2,2), white may take
it from (1,2)) and a ko in row 4 the other way round (white's stone on (1,4), black may take it from (2,4)), black to move, a quiet
history.  Under rules = 0 nobody may connect a ko, so every mover has exactly ONE candidate or none: B (2,4), W (1,2), B pass,
W (1,4), B (2,2), W pass, and so on for ever -- never two passes in a row.  (At 5x5 the kos stand in rows 1 and 3, next to the corner
eyes, where the cuts also capture the corner stones; the line is longer but has one candidate per ply all the same.)  A simulation there does not depend on its draws, with
expand_at = 0 the tree grows one node per simulation along this line, and with more than 64 simulations depth 64 is reached and held.
THE RUNS (whole games at 5x5, 7x7 and 9x9; max_plies = 40 at 13x13 and 19x19, where the model would take too long):
  games     the empty board and an eye shape for both colours, two trees, komi2 = 0
  komi      positions with stones to capture, three trees (a half without a tree), an odd komi2, expand_at = 0
  pool      expand_at = 0 with max_nodes = 3: every tree is refused a node
  short     every position of the set, max_plies = 2, komi2 = 0 (one stone each on an empty board is a draw), expand_at = 0: games that end
            inside the tree
  nil       prior = 0 and rave_equiv = 0: plain means, no RAVE
  best      plain means again, three trees that favour different moves, with a seed per size (found with the model) at which in some row
            the most visited child is not the child with the most wins
  kos       `two_kos` under rules = 0 with 70 simulations of at most 80 plies"""
import functools

import numpy as np

from tests import playout_cases as PC
from tests import playout_model as PM
from tests import uct_model as UM

SIZES = UM.SIZES
DEFAULTS = dict(index=None, trees=1, sims=16, seed=0, rules=1, max_plies=0, komi2=0, expand_at=2, rave_equiv=64, prior=4, max_nodes=None)
BEST_SEED = {5: 60, 7: 62, 9: 96, 13: 61, 19: 142}


def two_kos(S):
    P = lambda x, y: y * S + x                                                           # noqa: E731
    b, w = PC._split(S)
    y1, y2 = (1, 3) if S == 5 else (2, 4)
    b = sorted(set(b) - {P(1, y1), P(1, y2)} | {P(2, y1)})
    w = sorted(set(w) - {P(2, y1), P(2, y2)} | {P(1, y2)})
    return b, w


@functools.lru_cache(maxsize=None)
def case_records(S):
    """(names, records): those of tests/playout_cases.py, then `two_kos`"""
    names, recs = PC.case_records(S)
    b, w = two_kos(S)
    extra = PM.build_record(S, b, w, False, None, None, np.random.RandomState(77 * S))
    return names + ("two_kos",), np.concatenate([recs, extra[None]])


def rows(S, *wanted):
    names = case_records(S)[0]
    return tuple(names.index(nm) for nm in wanted)


@functools.lru_cache(maxsize=None)
def runs(S):
    """{name: the arguments of uct_model.search after the records}"""
    cap = 0 if S <= 9 else 40
    R = len(case_records(S)[0])
    out = {
        "games": dict(index=rows(S, "empty", "empty_x", "eye_in1", "eye_in1_x"), trees=2, sims=24, seed=51, max_plies=cap),
        "komi": dict(index=rows(S, "ko_hole", "ko_hole_b_x", "full_but_two", "words_x"), trees=3, sims=16, seed=52, rules=0, max_plies=cap or 60,
                     komi2=2 * (S % 4) + 1, expand_at=0),
        "pool": dict(index=rows(S, "empty_x", "eye_edge1"), trees=2, sims=16, seed=53, max_plies=cap and 20, expand_at=0, max_nodes=3),
        "short": dict(index=tuple(range(R)), trees=1, sims=16, seed=54, max_plies=2, expand_at=0),
        "nil": dict(index=rows(S, "empty", "eye_corner1_x"), trees=2, sims=16, seed=55, max_plies=30, komi2=-3, rave_equiv=0, prior=0),
        "best": dict(index=tuple(sorted(rows(S, *[nm + x for nm in ("eye_not", "ko_hole", "ko_hole_b", "full_but_two", "eye_in2", "words") for x in ("", "_x")]))),
                     trees=3, sims=20, seed=BEST_SEED[S], max_plies=8, komi2=1, expand_at=1, rave_equiv=0, prior=0),
        "kos": dict(index=rows(S, "two_kos"), trees=1, sims=70, seed=56, rules=0, max_plies=80, expand_at=0),
    }
    return {k: dict(DEFAULTS, **v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def run_model(S, name, fault=None):
    """the model's outputs of one run, computed once and shared (read only)"""
    return UM.search(S, case_records(S)[1], fault=fault, **runs(S)[name])
