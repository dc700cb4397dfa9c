"""The case set of the securing-move tests: the constructed positions of tests/life_cases.py and the ones below, each drawn at the
smallest size at which it can go wrong and placed at every size against the edges it uses, in the colour / flag variants of
tests/life_cases.case_points (`_sb`: as drawn, black to play; `_sw`: as drawn, white to play; `_cb` / `_cw`: colours swapped) over
random words in planes 4..15 and in the padding; then positions of rule_shapes_S*.npz; and every 16th record of
tactics_cases.golden_records(), 26 positions of the five golden 19x19 games.  With side 0 the mover of `_sb` is black; with side 1
the mover of `_sw` is black too, but without `prev`: that pair is what shows the ko restriction and its absence on one position.
tests/test_secure_model_power.py shows what each case reaches and which fault switch of tests/secure_model.py it notices;
tests/test_gpu_secure.py runs the same records on the device.

X is the colour the pictures are about (black as drawn):
  straight_three     a three-point eye on the edge: only the middle point makes two eyes
  capture_makes_eye  one region of two empty points and two O stones in atari between them: the capturing stone splits it in two
  capture_opens_eye  a living group whose second eye is one empty point beside a plus of five O stones: capturing them is ALLOWED
                     and leaves a five-point region whose centre touches no stone, so the group's life is gone (gain < 0)
  connect            two chains with one eye each and the point that joins them (from 7x7 on the right chain closes its own eye;
                     at 5x5 it uses the right edge)
  ko_secure          capture_makes_eye with one O stone, and `prev` says that exactly one X stone vanished on the capturing point
  suicide            moves_cases' two-stone suicide: the stone on (1, 0) and the corner stone go
The rule shapes are late play-out positions with few empty points; 8 of them stand at every size (the model's cost grows with the
number of empty points, and the golden positions are the expensive ones)."""
import functools

import numpy as np

from tests import life_cases as LC
from tests import secure_model as M
from tests.tactics_cases import diagram, golden_records, rule_shape_records
from tests.tactics_model import build_record

SIZES = M.SIZES
RULE_SHAPES = 8
GOLDEN_EVERY = 16


@functools.lru_cache(maxsize=None)
def positions(S):
    """[(name, black, white, black one ply ago or None)] as drawn"""
    out = [(name, b, w, None) for name, b, w in LC.positions(S)]
    b, w = diagram(S, ["...X", "XXXX"])
    out.append(("straight_three", b, w, None))
    b, w = diagram(S, ["..OOX", "XXXXX"])
    out.append(("capture_makes_eye", b, w, None))
    b, w = diagram(S, ["X.OXX", "XOOOX", "XXOXX", ".XXX.", "XX..."])
    out.append(("capture_opens_eye", b, w, None))
    b, w = diagram(S, [".X.X.", "XX.XX"] if S == 5 else [".X.X.X", "XX.XXX"])
    out.append(("connect", b, w, None))
    b, w = diagram(S, ["..OX", "XXXX"])
    out.append(("ko_secure", b, w, sorted(b + [1])))
    b, w = diagram(S, ["X.O", "OO"])
    out.append(("suicide", b, w, None))
    return out


@functools.lru_cache(maxsize=None)
def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW]): the constructed positions in their four variants over a random pattern, then the rule
    shapes"""
    rng = np.random.RandomState(5000 * S + seed)
    names, recs = [], []
    for name, b, w, pb in positions(S):
        for swap in (False, True):
            for wtp in (False, True):
                names.append("%s_%s%s" % (name, "c" if swap else "s", "w" if wtp else "b"))
                bb, ww, pbb, pww = (w, b, None, pb) if swap else (b, w, pb, None)
                recs.append(build_record(S, bb, ww, wtp, pbb, pww, rng))
    shapes = rule_shape_records(S)[:RULE_SHAPES]
    names += ["shape_%d" % i for i in range(len(shapes))]
    return names, np.concatenate([np.stack(recs), shapes])


@functools.lru_cache(maxsize=None)
def case_model(S, side):
    """the model's outputs on case_records(S), computed once and shared (read only)"""
    return M.secure(S, case_records(S)[1], side=side)


@functools.lru_cache(maxsize=None)
def golden_sample():
    """every 16th record of tactics_cases.golden_records() (itself every fourth record of the five golden 19x19 games)"""
    return golden_records()[::GOLDEN_EVERY].copy()


@functools.lru_cache(maxsize=None)
def golden_model(side):
    return M.secure(19, golden_sample(), side=side)
