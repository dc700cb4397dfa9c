"""Constructed rule positions (tests/golden/rule_shapes_S*.npz, gen_golden.py child_rule_shapes) and a plain restatement of
the set logic of csrc/sgo_rows.hpp / sgo_bits.hpp on Python integers, one per board row.

The restatement exists to measure the fixture, not to check the kernels: it counts the trips of the row-Jacobi flood fill
(rows::Board::flood: every row takes its vertical neighbours, then finishes its runs with the carry trick, until no row
changes), says which branches of legal_core a position reaches, and carries FAULT SWITCHES -- each the kind of slip the
kernels could hold -- so that tests/test_rule_shapes.py can show that the fixture notices them."""
import functools

import numpy as np

from tests.helpers import load, sha8

SIZES = (5, 7, 9, 13, 19)
# fill_capped: the flood stops after the deepest trip count the played-out goldens need; nl_ge1: a remaining group is
# capturable at ">= 1" liberties; while_if: only the first remaining group is looked at; single_ge1: "at least one" empty
# neighbour in the single-stone path; ko_ge1: ko applied when one OR MORE stones vanished; no_suicide_after_capture: the
# own group is not examined when the move captured
FAULTS = ("fill_capped", "nl_ge1", "while_if", "single_ge1", "ko_ge1", "no_suicide_after_capture")
SWAP_INDEX = [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 15, 14]


class Shapes(object):
    pass


@functools.lru_cache(maxsize=None)
def load_shapes(S):
    """The fixture of one size as arrays: boards int32 [P][S][S][17], legal uint8 [P][A] (1 = illegal), winner [P][3],
    plays (pos, a, colour, mover, hash, legal_hash)."""
    z = load("rule_shapes_S%d.npz" % S)
    assert int(z["size"]) == S
    N, A = S * S, S * S + 1
    f = Shapes()
    f.S, f.N, f.A, f.komi = S, N, A, float(z["komi"])
    f.names = bytes(z["names"]).decode().split("\n")
    planes = np.unpackbits(z["planes"], axis=-1)[..., :N]
    P = planes.shape[0]
    f.P = P
    f.boards = np.zeros((P, S, S, 17), dtype=np.int32)
    for k in range(4):
        f.boards[..., k] = planes[:, k].reshape(P, S, S)
    f.colour = z["colour"].astype(np.int32)
    f.boards[..., 16] = f.colour[:, None, None]
    f.legal = np.unpackbits(z["legal"], axis=-1)[:, :A]
    f.winner = z["winner"]
    f.play_pos = z["play_pos"].astype(np.int64)
    f.play_a = z["play_a"].astype(np.int32)
    f.play_colour = z["play_colour"].astype(np.int32)
    f.play_mover = z["play_mover"].astype(np.int32)
    f.play_hash = z["play_hash"]
    f.play_legal_hash = z["play_legal_hash"]
    f.K = len(f.play_pos)
    assert len(f.names) == P
    return f


# ---- rows of bits ---------------------------------------------------------------------------------------------------------
def rows_of(plane):
    S = plane.shape[0]
    return [int(v) for v in ((plane != 0).astype(np.int64) << np.arange(S)).sum(axis=1)]


def plane_of(rows, S):
    return ((np.array(rows, dtype=np.int64)[:, None] >> np.arange(S)) & 1).astype(np.int32)


def _brev(v):
    return int("{:032b}".format(v)[::-1], 2)


def nbr4(a, M):
    S = len(a)
    return [(((a[y] << 1) | (a[y] >> 1)) | (a[y - 1] if y else 0) | (a[y + 1] if y < S - 1 else 0)) & M for y in range(S)]


def row_fill(s, m, mrev):
    """sgo_bits.hpp row_fill: s grows to the ends of the runs of m it touches (the add ripples through a run)."""
    up = (((m + s) ^ m) & m) | s
    sr = _brev(up)
    dn = ((((mrev + sr) & 0xFFFFFFFF) ^ mrev) & mrev) | sr
    return _brev(dn)


def flood(x, m, cap=None):
    """rows::Board::flood.  Returns (set, trips); trips counts the last, unchanged one as the kernel's loop does."""
    S = len(x)
    mrev = [_brev(v) for v in m]
    trips = 0
    while cap is None or trips < cap:
        trips += 1
        new = []
        for y in range(S):
            s = x[y] | (((x[y - 1] if y else 0) | (x[y + 1] if y < S - 1 else 0)) & m[y])
            new.append(row_fill(s, m[y], mrev[y]) if s else 0)
        if new == x:
            break
        x = new
    return x, trips


def _note(st, kind, trips):
    if st is not None and trips > st.get(kind, 0):
        st[kind] = trips


def legal_variants(S, own, opp, prev, st=None, cap=None):
    """rows::Board::legal on rows of bits.  Returns {variant: rows of LEGAL points} for 'none' and the legal-set faults (all
    share the code before the branch they alter); st collects trips and which branches ran."""
    M = (1 << S) - 1
    emp = [~(own[y] | opp[y]) & M for y in range(S)]
    t0 = nbr4(emp, M)
    e1 = [emp[y] & t0[y] for y in range(S)]
    c = [emp[y] & ~t0[y] for y in range(S)]
    names = ("none", "nl_ge1", "while_if", "single_ge1")
    lg = {k: list(e1) for k in names}
    n_rem, two_lib = 0, False
    if any(c):
        t = nbr4(e1, M)
        safe, trips = flood([opp[y] & t[y] for y in range(S)], opp, cap)
        _note(st, "stone", trips)
        r = [opp[y] & ~safe[y] for y in range(S)]
        fr = nbr4(opp, M)
        s1, s1b = [], []
        for y in range(S):
            U, D = (emp[y - 1] if y else 0), (emp[y + 1] if y < S - 1 else 0)
            Lf, Rt = (emp[y] << 1) & M, emp[y] >> 1
            x1, a1, x2, a2 = U ^ D, U & D, Lf ^ Rt, Lf & Rt
            one = (x1 ^ x2) & ~((a1 & x2) | (a2 & x1))
            single = r[y] & ~fr[y]
            s1.append(single & one)
            s1b.append(single & (U | D | Lf | Rt))
            r[y] &= ~single
        n1, n1b = nbr4(s1, M), nbr4(s1b, M)
        for k in names:
            for y in range(S):
                lg[k][y] |= (n1b if k == "single_ge1" else n1)[y] & emp[y]
        while any(r):
            first = next(y for y in range(S) if r[y])
            g, trips = flood([(r[y] & -r[y]) if y == first else 0 for y in range(S)], r, cap)
            _note(st, "stone", trips)
            lib = nbr4(g, M)
            lib = [lib[y] & emp[y] for y in range(S)]
            nl = sum(bin(v).count("1") for v in lib)
            two_lib = two_lib or nl == 2
            for k in names:
                if (nl >= 1 if k == "nl_ge1" else nl == 1) and not (k == "while_if" and n_rem):
                    for y in range(S):
                        lg[k][y] |= lib[y]
            r = [r[y] & ~g[y] for y in range(S)]
            n_rem += 1
    if st is not None:
        st["remaining"] = max(st.get("remaining", 0), n_rem)
        st["two_lib_c"] = st.get("two_lib_c", False) or two_lib
    gone = [prev[y] & ~own[y] for y in range(S)]
    kc = sum(bin(v).count("1") for v in gone)
    lg["ko_ge1"] = list(lg["none"])
    for k in lg:
        if kc == 1 or (k == "ko_ge1" and kc >= 1):
            lg[k] = [lg[k][y] & ~gone[y] for y in range(S)]
    return lg


def advance(S, own, opp, a, st=None, cap=None, no_suicide_after_capture=False):
    """rows::Board::advance on an empty point (or the pass a = S*S): the stone, the captures, the executed suicide."""
    if a >= S * S:
        return own, opp
    M = (1 << S) - 1
    my, mx = divmod(a, S)
    pb = [(1 << mx) if y == my else 0 for y in range(S)]
    assert not (own[my] | opp[my]) & pb[my]
    np_ = nbr4(pb, M)
    own = [own[y] | pb[y] for y in range(S)]
    emp = [~(own[y] | opp[y]) & M for y in range(S)]
    captured = False
    if any(np_[y] & opp[y] for y in range(S)):
        t = nbr4(emp, M)
        alive, trips = flood([opp[y] & t[y] for y in range(S)], opp, cap)
        _note(st, "stone", trips)
        dead = [opp[y] & ~alive[y] for y in range(S)]
        capt, trips = flood([dead[y] & np_[y] for y in range(S)], dead, cap)
        _note(st, "stone", trips)
        captured = any(capt)
        opp = [opp[y] & ~capt[y] for y in range(S)]
        emp = [emp[y] | capt[y] for y in range(S)]
    if not any(np_[y] & emp[y] for y in range(S)) and not (captured and no_suicide_after_capture):
        t = nbr4(emp, M)
        alive, trips = flood([own[y] & t[y] for y in range(S)], own, cap)
        _note(st, "stone", trips)
        if not any(alive[y] & pb[y] for y in range(S)):
            dead = [own[y] & ~alive[y] for y in range(S)]
            sg, trips = flood([pb[y] & dead[y] for y in range(S)], dead, cap)
            _note(st, "stone", trips)
            own = [own[y] & ~sg[y] for y in range(S)]
    return own, opp


def make_play(board, a, colour, st=None, cap=None, no_suicide_after_capture=False):
    """play.py:226-242 on a board tensor [1][S][S][17] with the stone logic above.  Returns (new tensor, mover)."""
    b = board.copy()
    S = b.shape[1]
    if colour and colour != b[0, 0, 0, 16]:
        b[..., :16] = b[..., SWAP_INDEX]
        b[..., 16] = -b[..., 16]
    mover = int(b[0, 0, 0, 16])
    b[..., 2:16] = b[..., 0:14].copy()
    own, opp = advance(S, rows_of(b[0, :, :, 0]), rows_of(b[0, :, :, 1]), a, st, cap, no_suicide_after_capture)
    b[0, :, :, 0], b[0, :, :, 1] = plane_of(own, S), plane_of(opp, S)
    b[..., :16] = b[..., SWAP_INDEX]
    b[..., 16] = -mover
    return b, mover


def legal_masks(board, st=None, cap=None):
    """{variant: uint8 [A] in the reference's convention (1 = illegal, pass 0)} of a board tensor."""
    S = board.shape[1]
    lg = legal_variants(S, rows_of(board[0, :, :, 0]), rows_of(board[0, :, :, 1]), rows_of(board[0, :, :, 2]), st, cap)
    return {k: np.append(1 - plane_of(v, S).reshape(-1), 0).astype(np.uint8) for k, v in lg.items()}


def score(board, komi, st=None, cap=None):
    """score_core: (winner, black, white + komi)."""
    S = board.shape[1]
    M = (1 << S) - 1
    tp = int(board[0, 0, 0, 16])
    black, white = rows_of(board[0, :, :, 0 if tp == 1 else 1]), rows_of(board[0, :, :, 1 if tp == 1 else 0])
    emp = [~(black[y] | white[y]) & M for y in range(S)]
    pts = []
    for mine in (black, white):
        t = nbr4(mine, M)
        reach, trips = flood([t[y] & emp[y] for y in range(S)], emp, cap)
        _note(st, "empty", trips)
        pts.append(reach)
    bp = sum(bin(black[y]).count("1") + bin(pts[0][y] & ~pts[1][y]).count("1") for y in range(S))
    wp = sum(bin(white[y]).count("1") + bin(pts[1][y] & ~pts[0][y]).count("1") for y in range(S)) + komi
    return (1 if bp > wp else 0 if bp == wp else -1), bp, wp


# ---- running a fixture through the restatement ------------------------------------------------------------------------------
def _tally(fails, st, board, want_mask, want_score, plays, komi, cap):
    """One position: its legal mask, its score (when recorded) and plays [(a, colour, want_hash)], under every fault."""
    local = {}
    masks = legal_masks(board, local)
    capped = masks
    if cap is not None and local.get("stone", 0) > cap:
        capped = legal_masks(board, None, cap)
    for k in FAULTS[1:5]:
        fails[k] += int(not np.array_equal(masks[k], want_mask))
    fails["none"] += int(not np.array_equal(masks["none"], want_mask))
    fails["fill_capped"] += int(not np.array_equal(capped["none"], want_mask))
    if want_score is not None:
        sl = {}
        got = score(board, komi, sl)
        fails["none"] += int(got != want_score)
        if cap is not None and sl.get("empty", 0) > cap:
            got = score(board, komi, None, cap)
        fails["fill_capped"] += int(got != want_score)
        _note(st, "empty", sl.get("empty", 0))
    for a, colour, want in plays:
        pl = {}
        b2, _ = make_play(board, a, colour, pl)
        fails["none"] += int(not np.array_equal(sha8(b2), want))
        b3, _ = make_play(board, a, colour, None, None, True)
        fails["no_suicide_after_capture"] += int(not np.array_equal(sha8(b3), want))
        if cap is not None and pl.get("stone", 0) > cap:
            b2, _ = make_play(board, a, colour, None, cap)
        fails["fill_capped"] += int(not np.array_equal(sha8(b2), want))
        _note(local, "stone", pl.get("stone", 0))
    _note(st, "stone", local.get("stone", 0))
    st["remaining_ge2"] = st.get("remaining_ge2", 0) + int(local.get("remaining", 0) >= 2)
    st["two_lib_c"] = st.get("two_lib_c", 0) + int(local.get("two_lib_c", False))
    st["cases"] = st.get("cases", 0) + 1 + int(want_score is not None) + len(plays)


def run_shapes(S, cap):
    """(failing cases per fault and for 'none', stats) of rule_shapes_S<S>.npz; a case is one mask, one score or one play."""
    f = load_shapes(S)
    fails, st = dict.fromkeys(("none",) + FAULTS, 0), {}
    by_pos = [[] for _ in range(f.P)]
    for k in range(f.K):
        by_pos[f.play_pos[k]].append((int(f.play_a[k]), int(f.play_colour[k]), f.play_hash[k]))
    for p in range(f.P):
        w = f.winner[p]
        _tally(fails, st, f.boards[p:p + 1], f.legal[p], (int(w[0]), int(w[1]), float(w[2])), by_pos[p], f.komi, cap)
    return fails, st


# the played-out rules games of each size (gen_golden.py child_rules): the yardstick of what playouts reach
PLAYED_OUT = {5: ["rules_S5.npz", "rules_S5_seed101.npz"], 7: ["rules_S7.npz"], 9: ["rules_S9.npz", "rules_S9_seed202.npz"],
              13: ["rules_S13.npz", "rules_S13_seed303.npz"], 19: ["rules_S19.npz"]}


def run_goldens(S, cap):
    """The same over the played-out games of rules_S<S>*.npz, every position taken from the oracle's replay."""
    from oracle import oracle as ora
    fails, st = dict.fromkeys(("none",) + FAULTS, 0), {}
    A = S * S + 1
    for name in PLAYED_OUT[S]:
        z = load(name)
        komi = float(z["komi"])
        for gi in range(int(z["n_games"])):
            p = "g%02d_" % gi
            board, _ = ora.game_init(S)
            moves, masks, hashes = z[p + "moves"], z[p + "masks"], z[p + "hashes"]
            full_at = list(z[p + "full_at"])
            for ply in range(len(moves) + 1):
                want_score = None
                if ply in full_at:
                    w = z[p + "winners"][full_at.index(ply)]
                    want_score = (int(w[0]), int(w[1]), float(w[2]))
                plays = []
                if ply < len(moves):
                    x, y, colour = (int(v) for v in moves[ply])
                    plays = [(y * S + x if y != S else S * S, colour, hashes[ply + 1])]
                _tally(fails, st, board, np.unpackbits(masks[ply])[:A], want_score, plays, komi, cap)
                if plays:
                    ora.make_play(x, y, board, None if colour == 0 else colour)
    return fails, st
