"""The case set of the superko tests.  A case is a run of consecutive records (a "game": positions constructed directly or played out
with the model's ply) plus rows (r, f) into it; all games of one size lie back to back in ONE record array, as a replay lays them
out, so that every game has neighbours a wrong history bound would reach.  Every game is given for both colours (the second with
black and white exchanged and the flag flipped) over random words in planes 4..15 and in the padding.  The shapes are drawn into
the corners, so the set stands at 5x5 (without the triple ko, which needs 7x7) and again at every larger size.
tests/test_superko_model_power.py shows that the set notices every fault switch of tests/superko_model.py;
tests/test_gpu_superko.py runs the same records on the device."""
import functools

import numpy as np

from tests import superko_model as SM
from tests.tactics_cases import diagram
from tests.tactics_model import build_record

SIZES = SM.SIZES


def _points(mask, N):
    return [a for a in range(N) if (mask >> a) & 1]


def play_out(S, black, white, wtp, moves):
    """[(black, white, white_to_play)] point lists: the start and the position after every move (N = a pass), by the model's ply"""
    N = S * S
    out = [(sorted(black), sorted(white), bool(wtp))]
    for a in moves:
        b, w, t = out[-1]
        if a == N:
            out.append((b, w, not t))
        else:
            b2, w2, t2 = SM.after_position(S, build_record(S, b, w, t), a)
            out.append((_points(b2, N), _points(w2, N), t2))
    return out


class _Set(object):
    def __init__(self, S):
        self.S, self.rng = S, np.random.RandomState(7000 * S)
        self.recs, self.rows, self.names, self.bases = [], [], [], {}

    def game(self, name, positions, rows):
        """both colour versions of a game; rows [(r, f)] relative to its first record (they may point outside it)"""
        for swap in (False, True):
            base = len(self.recs)
            self.bases[name + ("_w" if swap else "_b")] = base
            prev = None
            for b, w, t in positions:
                if swap:
                    b, w, t = w, b, not t
                pb, pw = prev if prev is not None else (b, w)
                self.recs.append(build_record(self.S, b, w, t, pb, pw, self.rng))
                prev = (b, w)
            for r, f in rows:
                self.names.append("%s_%s_%d_%d" % (name, "w" if swap else "b", r, f))
                self.rows.append((base + r, base + f))


@functools.lru_cache(maxsize=None)
def case_set(S):
    """(records uint32 [R, 16 * NW], rows int32 [n, 2] of (r, f), row names, {game name: first record})"""
    N = S * S
    P = lambda x, y: y * S + x                                                           # noqa: E731
    cs = _Set(S)
    # simple ko on the top edge: black takes (3,0), white's recapture on (2,0) gives the first record again: back 1, not in extra
    b, w = diagram(S, [".XO.O", "..XO."])
    ko = play_out(S, b, w, False, [P(3, 0)])
    cs.game("ko", ko, [(1, 0), (1, 1), (0, 0)])
    # sending two, returning one in the corner: black adds (0,0) to (1,0), white takes both on (2,0), black retakes on (1,0) and the
    # stones are those of two plies back with the OTHER side to move: extra with back 2 under rule 0, absent under rule 1
    b, w = diagram(S, [".X.X", "OOX"])
    cs.game("send_two", play_out(S, b, w, False, [P(0, 0), P(2, 0)]), [(2, 0), (2, 1), (2, 2), (1, 0)])
    if S >= 7:
        # triple ko: edge kos on the top, the bottom and the right side.  L holds white's stone (state w) or R holds black's (b).
        m = S - 1
        walls_b = [P(0, 0), P(1, 1), P(0, m), P(1, m - 1), P(m, 1), P(m - 1, 2)]
        walls_w = [P(3, 0), P(2, 1), P(3, m), P(2, m - 1), P(m, 4), P(m - 1, 3)]
        L, Rt = [P(1, 0), P(1, m), P(m, 2)], [P(2, 0), P(2, m), P(m, 3)]
        # (b, w, w) with black to move; black takes B, white A, black C, white B, black A; then white on C would close the cycle
        start_b, start_w = walls_b + [Rt[0]], walls_w + [L[1], L[2]]
        seq = play_out(S, start_b, start_w, False, [Rt[1], L[0], Rt[2], L[1], Rt[0]])
        assert len(seq[-1][0]) == len(start_b) + 1 and len(seq[-1][1]) == len(start_w) - 1
        cs.game("triple_ko", seq, [(5, 0), (5, 1), (4, 0), (3, 0)])
    # passes: the same stones three times, the flag alternating; the single-stone suicide on (0,0) gives the current stones again
    b, w = diagram(S, [".O.", "O..", "..X"])
    cs.game("passes", [(b, w, False), (b, w, True), (b, w, False)], [(1, 0), (2, 0), (2, 1), (2, 2), (0, 0)])
    # a two-stone suicide on (1,0) whose result is the first record
    b, w = diagram(S, ["X.O", "OO"])
    cs.game("suicide2", [([], w, True), (b, w, True), (b, w, False)], [(2, 0), (2, 1), (2, 2)])
    # quiet points: the history holds the current stones and one isolated stone -- on the last point of the board, beside a set
    # flag (at 5x5 they share the plane's only word), in the centre and on an edge; the same record twice: the later one wins
    b, w = diagram(S, ["X.", ".O"])
    q = [N - 1, P(S // 2, S // 2), P(S - 1, 1)]
    cs.game("quiet", [(b + [q[0]], w, True), (b + [q[1]], w, True), (b + [q[1]], w, True), (b + [q[2]], w, False), (b, w, False)],
            [(4, 0), (4, 1), (4, 2), (4, 3), (4, 4)])
    # a contact point without a capture: (3,2) next to black's (2,2) and white's (3,1)
    b, w = diagram(S, ["....", "...O", "..X."])
    cs.game("contact", [(sorted(b + [P(3, 2)]), w, True), (b, w, True), (b, w, False)], [(2, 0), (2, 1)])
    # neighbours: the games before and behind hold what (2,2) would give; the game between them is one record long
    b, w = diagram(S, ["X", ".O"])
    cs.game("neighbours", [(b + [P(2, 2)], w, True), (b, w, False), (b + [P(2, 2)], w, True)], [(1, 1), (1, 0), (2, 1)])
    # degenerate boards
    cs.game("empty", [([], [], False)], [(0, 0)])
    cs.game("full", [(list(range(N)), [], False), (list(range(N)), [], True)], [(1, 0)])
    # every point but the centre holds a black stone.  White there captures them all; black there takes its own N stones off,
    # and the empty board is the record before
    most = [a for a in range(N) if a != P(S // 2, S // 2)]
    cs.game("full_minus_one", [(most, [], True)], [(0, 0)])
    cs.game("board_suicide", [([], [], True), (most, [], False)], [(1, 0), (1, 1)])
    recs = np.stack(cs.recs)
    R = len(recs)
    # zero rows: the index out of range on both sides, f < 0, f > r
    for name, row in (("below", (-1, 0)), ("above", (R, 0)), ("far_above", (2 ** 31 - 1, 0)), ("far_below", (-2 ** 31, 0)), ("f_negative", (3, -1)),
                      ("f_behind", (3, 4)), ("f_far", (3, 2 ** 31 - 1))):
        cs.names.append("zero_" + name)
        cs.rows.append(row)
    return recs, np.array(cs.rows, np.int64), list(cs.names), dict(cs.bases)


@functools.lru_cache(maxsize=None)
def case_model(S, rule):
    """the model's outputs on the rows of case_set(S), computed once and shared (read only)"""
    recs, rows, _, _ = case_set(S)
    return SM.superko(S, recs, rows, rule)


# ---- the long history at 19x19 ----------------------------------------------------------------------------------------------------
LONG_S = 19


@functools.lru_cache(maxsize=None)
def long_history():
    """(records [H + 1 + 2, 16 * NW], rows, names) at 19x19 with H = SGO_SUPERKO_MAX_HISTORY(19): one game of H + 1 records built from
    pairs "a position, the same position after a pass" with stones that change from pair to pair, its last record the current
    one; then an empty board twice.  What one more black stone gives stands at record 0 (outside the window when f = 0: the history
    is one record too long), at record 1 (the oldest record of the window), at record 2 again and just before the end; the
    current stones stand at record 3 with the same side to move."""
    S, N = LONG_S, LONG_S * LONG_S
    H = SM.max_history(S)
    rng = np.random.RandomState(1919)
    P = lambda x, y: y * S + x                                                           # noqa: E731
    base_b, base_w = diagram(S, ["....", ".X..", "..O."])
    free = [a for a in range(N) if a not in base_b and a not in base_w]
    recs = []
    for j in range(H + 1):
        k = j // 2                                                   # the pair: two stones that walk over the board
        e1, e2 = free[(7 * k) % len(free)], free[(7 * k + 3 + k // len(free)) % len(free)]
        if e1 == e2:
            e2 = free[(free.index(e1) + 1) % len(free)]
        recs.append([sorted(base_b + [e1]), sorted(base_w + [e2]), j % 2 == 1])
    a0, a1, a2 = P(10, 10), P(18, 18), P(0, 18)
    recs[0] = [sorted(base_b + [a0]), base_w, True]
    recs[1] = [sorted(base_b + [a1]), base_w, True]
    recs[2] = [sorted(base_b + [a1]), base_w, False]
    recs[3] = [base_b, base_w, False]
    recs[H - 1] = [sorted(base_b + [a2]), base_w, True]
    recs[H] = [base_b, base_w, False]
    out, prev = [], None
    for b, w, t in recs + [[[], [], False], [[], [], True]]:
        pb, pw = prev if prev is not None else (b, w)
        out.append(build_record(S, b, w, t, pb, pw, rng))
        prev = (b, w)
    rows = [(H, 0), (H, 1), (H, 2), (H, 3), (H + 1, H + 1), (H + 2, H + 1), (H - 1, 0)]
    names = ["one_too_long", "exactly_max", "short_by_one", "short_by_two", "empty_alone", "empty_after_pass", "full_window_inside"]
    return np.stack(out), np.array(rows, np.int64), names, (a0, a1, a2)


@functools.lru_cache(maxsize=None)
def long_model(rule):
    recs, rows, _, _ = long_history()
    return SM.superko(LONG_S, recs, rows, rule)


# ---- the golden 19x19 games --------------------------------------------------------------------------------------------------------
GOLDEN_STRIDE, GOLDEN_TAIL = 40, 6


@functools.lru_cache(maxsize=None)
def golden_games():
    """[[(action, colour)]] of the five golden 19x19 games"""
    from tests.helpers import load
    z = load("sgf_S19.npz")
    return [[(361 if y >= 19 else int(y) * 19 + int(x), int(c)) for x, y, c in z["g%02d_moves" % gi]] for gi in range(5)]


@functools.lru_cache(maxsize=None)
def golden_sample():
    """(records of the five games as a replay lays them out, rows (r, f)): the last six records of each game and every 40th"""
    from tests.tactics_cases import golden_records
    recs = golden_records(1)
    rows, base = [], 0
    for g in golden_games():
        n = len(g) + 1
        keep = sorted(set(range(0, n, GOLDEN_STRIDE)) | set(range(max(0, n - GOLDEN_TAIL), n)))
        rows += [(base + j, base) for j in keep]
        base += n
    assert base == len(recs)
    return recs, np.array(rows, np.int64)


@functools.lru_cache(maxsize=None)
def golden_model(rule):
    recs, rows = golden_sample()
    return SM.superko(19, recs, rows, rule)
