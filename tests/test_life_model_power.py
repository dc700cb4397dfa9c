"""CPU: the model of unconditional life (tests/life_model.py) is exact -- on tiny boards its alive set equals what an independent
brute force cannot capture -- it says what include/sgo.h states on the constructed cases (tests/life_cases.py), the cases reach what
they were built for, and every fault switch of the model changes a compared value of a named case -- so a green run of
tests/test_gpu_life.py means something."""
import itertools

import numpy as np
import pytest

from tests import life_cases as LC
from tests import life_model as M

# fault -> (board size, case name): the case whose compared values the switch changes
NOTICED_BY = {
    "one_vital_enough": (5, "one_eye_sb"),
    "some_empty_adjacent": (5, "corner3_sb"),
    "regions_not_removed": (7, "cascade_sb"),
    "single_round": (7, "cascade_cw"),
    "all_kept_regions_are_territory": (5, "wall_sb"),
    "empty_less_region_vital": (5, "illegal_corner_sb"),
    "stones_must_be_adjacent": (5, "dead_stone_cb"),
    "region_8_connected": (5, "two_eyes_sw"),
    "flag_as_stone": (5, "edge_eyes_sw"),
    "padding_read": (5, "edge_eyes_cb"),
}


# ---- the brute force: the opponent plays any sequence of legal moves while X always passes ------------------------------------
class Brute(object):
    """Boards as bit masks (point a = bit a).  capturable(X, O) = the X stones some sequence of O moves removes: a move is a stone
    on an empty point; X chains left without a liberty go first; a move whose own chain then has no liberty is not allowed.  O
    stones are never captured (X passes), so every move adds one: the state graph has no cycle and is memoised whole."""

    def __init__(self, S):
        self.S, self.N = S, S * S
        self.nb = []
        for a in range(self.N):
            x, y = a % S, a // S
            self.nb.append(sum(1 << ((y + dy) * S + x + dx) for dx, dy in M.N4 if 0 <= x + dx < S and 0 <= y + dy < S))
        self.memo = {}

    def grow(self, v):
        out, a = 0, 0
        while v:
            if v & 1:
                out |= self.nb[a]
            v >>= 1
            a += 1
        return out

    def chain(self, seed, m):
        x = seed
        while True:
            t = (x | self.grow(x)) & m
            if t == x:
                return x
            x = t

    def chains(self, m):
        while m:
            c = self.chain(m & -m, m)
            yield c
            m &= ~c

    def legal(self, X, O):
        """every chain of either colour has a liberty"""
        emp = ~(X | O) & ((1 << self.N) - 1)
        return all(self.grow(c) & emp for m in (X, O) for c in self.chains(m))

    def capturable(self, X, O):
        key = (X, O)
        if key in self.memo:
            return self.memo[key]
        full = (1 << self.N) - 1
        out = 0
        for a in range(self.N):
            p = 1 << a
            if (X | O) & p:
                continue
            O2, X2 = O | p, X
            emp = full & ~(X | O2)
            for c in list(self.chains(X)):
                if not self.grow(c) & emp:
                    X2 &= ~c
            emp = full & ~(X2 | O2)
            if not self.grow(self.chain(p, O2)) & emp:
                continue
            out |= (X & ~X2) | self.capturable(X2, O2)
        self.memo[key] = out
        return out


def _pts(v):
    return [a for a in range(v.bit_length()) if (v >> a) & 1]


def _check_exact(br, X, O):
    want = X & ~br.capturable(X, O)
    alive = M.benson(br.S, _pts(X), _pts(O))[0]
    assert sum(1 << a for a in alive) == want, (br.S, _pts(X), _pts(O), sorted(alive), _pts(want))
    return want != 0


def test_exact_on_every_legal_3x3_position():
    """alive_X is exactly the set of X stones no sequence of opponent moves removes: all 12 675 legal positions of the 3x3 board,
    both colours of each (883 positions have alive black stones)"""
    br = Brute(3)
    legal = with_alive = 0
    for cells in itertools.product((0, 1, 2), repeat=9):
        X = sum(1 << a for a, c in enumerate(cells) if c == 1)
        O = sum(1 << a for a, c in enumerate(cells) if c == 2)
        if not br.legal(X, O):
            continue
        legal += 1
        with_alive += _check_exact(br, X, O)
    assert legal == 12675 and with_alive == 883


def test_exact_on_sampled_4x4_positions():
    """a seeded sample of legal 4x4 positions with at most 9 points that are not X, drawn until 300 are legal; the share with alive
    stones is asserted so that the sample cannot go empty"""
    br = Brute(4)
    rng = np.random.RandomState(44)
    done = with_alive = 0
    while done < 300:
        k = rng.randint(1, 10)                                   # points that are not X
        free = rng.choice(16, k, replace=False)
        X = (1 << 16) - 1
        O = 0
        for a in free:
            X &= ~(1 << int(a))
            if rng.rand() < 0.35:
                O |= 1 << int(a)
        if not X or not br.legal(X, O):
            continue
        done += 1
        with_alive += _check_exact(br, X, O)
    assert with_alive >= 50


# ---- the case set ---------------------------------------------------------------------------------------------------------------
def _row(S, name, fault=None):
    names, recs = LC.case_records(S)
    i = names.index(name)
    if fault is None:
        m = LC.case_model(S)
        return m["sets"][i], m["counts"][i], m["rounds"][i]
    m = M.life(S, recs[i:i + 1], fault=fault)
    return m["sets"][0], m["counts"][0], m["rounds"][0]


@pytest.mark.parametrize("fault", sorted(NOTICED_BY))
def test_fault_switch_changes_a_named_case(fault):
    S, name = NOTICED_BY[fault]
    good, bad = _row(S, name), _row(S, name, fault)
    assert not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])), (fault, name)


def test_every_switch_is_shown():
    """no switch of the model is inert: each has its named case"""
    assert set(M.FAULTS) == set(NOTICED_BY)


def test_small_cases_say_what_the_header_states():
    S, N = 5, 25
    c = lambda name: _row(S, name)[1].tolist()                                           # noqa: E731
    assert c("empty_sb") == [0, 0, 0, 0, 0, 0, N, 0] and c("empty_sw") == c("empty_sb")
    assert c("two_eyes_sb") == [7, 0, 2, 0, 0, 0, N - 9, 9]
    assert c("one_eye_sb") == [0, 0, 0, 0, 0, 0, N, 0] and c("private_sb") == c("one_eye_sb")
    # two chains, eight stones, the two shared eyes: without chain B chain A is not alive
    assert c("shared_sb") == [8, 0, 2, 0, 0, 0, N - 10, 10]
    names = dict((n, (b, w)) for n, b, w in LC.positions(S))
    b, _ = names["shared"]
    assert len(M.components(S, b, N)) == 2
    a_only = max(M.components(S, b, N), key=len)
    assert M.benson(S, a_only, [])[0] == set()
    # the corner of three points is vital to no one; with the white stone on its corner point it is, and the stone is dead
    assert c("corner3_sb") == [0, 0, 0, 0, 0, 0, N, 0]
    assert c("dead_stone_sb") == [11, 0, 4, 0, 1, 0, N - 15, 15] and c("dead_stone_cw") == [0, 11, 0, 4, 0, 1, N - 15, -15]
    # the living wall: 13 stones and two eyes; the ten open points above are no territory
    sets, counts, _ = _row(S, "wall_sw")
    assert counts.tolist() == [13, 0, 2, 0, 0, 0, 10, 15]
    assert M.points_of(sets[2], N) == [15, 17] and 24 in M.points_of(sets[0], N)         # the last point, beside the flag in one word
    assert c("settled_sb") == [13, 8, 2, 2, 0, 0, 0, 5] and c("settled_cw") == [8, 13, 2, 2, 0, 0, 0, -5]
    assert c("illegal_corner_sb") == [0, 0, 0, 0, 0, 0, N, 0]
    # 19x19: the blocks across the word boundaries; the lattice of chains in atari; a black stone without a liberty inside a
    # living white group is neither an eye nor territory
    sets, counts, _ = _row(19, "word_bounds_sb")
    assert counts.tolist() == [26, 13, 4, 2, 0, 0, 361 - 45, 15]
    assert M.points_of(sets[2], 361) == [31, 33, 338, 340] and M.points_of(sets[3], 361) == [63, 65]
    assert {32, 360} <= set(M.points_of(sets[0], 361)) and 64 in M.points_of(sets[1], 361)
    assert _row(19, "lattice_sb")[1].tolist() == [0, 0, 0, 0, 0, 0, 361, 0]
    assert _row(19, "illegal_sb")[1].tolist() == [0, 18, 0, 2, 0, 0, 361 - 20, -20]


def test_cascade_and_snake_reach_their_round_counts():
    """the open diagonal takes S - 1 passes that remove something and one that does not; its last stones had two vital regions in
    the first pass (a single pass leaves them standing); the closed diagonal is alive in one pass"""
    for S in (7, 9, 13, 19):
        sets, counts, rounds = _row(S, "cascade_sb")
        assert rounds.tolist() == [S, 1] and not counts[:6].any()
        once = _row(S, "cascade_sb", "single_round")
        assert once[1][0] == 2 * (S - 1) - 2 and {S * S - 2, S * S - S - 1} <= set(M.points_of(once[0][0], S * S))
        assert _row(S, "cascade_cb")[2].tolist() == [1, S]
        assert _row(S, "diagonal_alive_sb")[1].tolist()[:4] == [2 * (S - 1), 0, S, 0]
    assert _row(19, "lattice_sb")[2].tolist() == [4, 4]


@pytest.mark.parametrize("S", M.SIZES)
def test_symmetries_colours_and_flag(S):
    """the eight tables of sgo_sym_lut permute the outputs, swapping the colours swaps them, the flag changes nothing, and no point
    is safe for both colours"""
    from tests.keys_model import luts
    N = S * S
    L = luts(S)
    pts = dict((n, (b, w)) for n, b, w, _ in LC.case_points(S))
    for name, b, w in LC.positions(S):
        base = M.point_life(S, b, w)
        assert not (base["alive"][0] | base["terr"][0]) & (base["alive"][1] | base["terr"][1]), name
        for k in range(8) if S <= 9 or name in ("cascade", "word_bounds", "illegal") else (3,):
            t = lambda s: {int(L[k, a]) for a in s}                                      # noqa: E731
            moved = M.point_life(S, sorted(t(b)), sorted(t(w)))
            assert moved["counts"] == base["counts"], (name, k)
            for c in (0, 1):
                assert moved["alive"][c] == t(base["alive"][c]) and moved["terr"][c] == t(base["terr"][c]), (name, k)
        sw = M.point_life(S, w, b)
        cb = base["counts"]
        assert sw["counts"] == [cb[1], cb[0], cb[3], cb[2], cb[5], cb[4], cb[6], -cb[7]] and sw["alive"] == base["alive"][::-1], name
        for tag in ("s", "c"):
            a, b2 = _row(S, "%s_%sb" % (name, tag)), _row(S, "%s_%sw" % (name, tag))
            assert np.array_equal(a[0], b2[0]) and np.array_equal(a[1], b2[1]), name
        assert pts[name + "_sb"] == (list(b), list(w))
    m = LC.case_model(S)
    assert not ((m["sets"][:, 0] | m["sets"][:, 2]) & (m["sets"][:, 1] | m["sets"][:, 3])).any()
    NW = (N + 31) // 32
    top = np.uint32(0xFFFFFFFF) << np.uint32(N & 31) if N & 31 else np.uint32(0)
    assert not (m["sets"][:, :, NW - 1] & top).any()                                     # bits a >= N are zero


def test_replayed_positions():
    """the share of replayed positions with a non-empty alive set, as tests/life_cases.py states it; the model's rounds on them"""
    for S, want in zip(M.SIZES, (16, 24, 24, 24, 24)):
        names = LC.case_records(S)[0]
        m = LC.case_model(S)
        shapes = [i for i, n in enumerate(names) if n.startswith("shape_")]
        assert len(shapes) == 24 and sum(bool(m["counts"][i][:2].any()) for i in shapes) == want
    g = LC.golden_model()
    assert len(g["counts"]) == 412 and int((g["counts"][:, :2].sum(axis=1) > 0).sum()) == 86
    assert int(g["rounds"].max()) == 5 and 2.4 < float(g["rounds"].mean()) < 2.7
    assert not ((g["sets"][:, 0] | g["sets"][:, 2]) & (g["sets"][:, 1] | g["sets"][:, 3])).any()
