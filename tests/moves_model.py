"""CPU model of the move-outcome table (include/sgo.h "move outcomes"), written from the header's text: a board is a Python list
with one entry per point (0 empty, 1 own, 2 opp), a chain is found with a stack, a ply lifts the opponent's chains without a
liberty and then the mover's own.  No bitboards, and no code of the package takes part; tests/test_moves_model_power.py ties the
model's ALLOWED bits and its positions after the ply to oracle.legal_moves / oracle.make_play.  Everything is integer: the GPU
results must match word for word.

FAULT SWITCHES -- each the kind of slip the kernel could hold (tests/test_moves_model_power.py shows which case notices which).
Model and test helper only; no library code reads them.
  capture_after_suicide  the mover's chain is judged (and lifted) before the opponent's chains are
  libs_before_lift       `libs` is counted with the captured stones still on the board
  weakest_without_a      `weakest` does not count the point itself as a liberty
  joined_stones          `joined` counts neighbouring own stones, not distinct chains
  ataris_anywhere        `ataris` / `atari_stones` count every opp chain of P' with one liberty, adjacent to the point or not
  allowed_not_suicide    ALLOWED is "empty, not suicide, not ko" instead of the project's rule
  ko_wrong_plane         `prev` is taken from the other colour's plane
  ko_at_side1            `prev` (the mover's plane) and the ko test are applied at side 1 as well
  flag_as_stone          the to-play flag is read as a black stone
  padding_read           bits >= N of planes 0 / 1 (other than the flag) are read as stones
  max_move_highest       max_capture_move is the highest point that reaches max_captured
  quiet_no_edge          a point without a stone among its neighbours gets libs = 4, at the edge and in the corner too

With flag_as_stone / padding_read the board is the STRIP the plane words form (width S, 32 * NW points), as a kernel reading the
words without a mask would see it; rows are reported for the points a < N only."""
import numpy as np

FAULTS = ("capture_after_suicide", "libs_before_lift", "weakest_without_a", "joined_stones", "ataris_anywhere", "allowed_not_suicide",
          "ko_wrong_plane", "ko_at_side1", "flag_as_stone", "padding_read", "max_move_highest", "quiet_no_edge")
SIZES = (5, 7, 9, 13, 19)
ALLOWED, OCCUPIED, KO, SUICIDE = 1, 2, 4, 8
EMPTY, OWN, OPP = 0, 1, 2
_NBRS = {}


def neighbours(S, area):
    """per point a < area the list of its 4-neighbours inside the area (N: the board; 32 * NW: the strip of the plane words)"""
    if (S, area) not in _NBRS:
        out = []
        for a in range(area):
            x, nb = a % S, []
            if x > 0:
                nb.append(a - 1)
            if x < S - 1 and a + 1 < area:
                nb.append(a + 1)
            if a - S >= 0:
                nb.append(a - S)
            if a + S < area:
                nb.append(a + S)
            out.append(nb)
        _NBRS[(S, area)] = out
    return _NBRS[(S, area)]


def chain(board, nbrs, a):
    """(the points of the chain on a, the set of its liberties); a holds a stone"""
    colour, seen, todo, libs = board[a], {a}, [a], set()
    while todo:
        p = todo.pop()
        for q in nbrs[p]:
            if board[q] == EMPTY:
                libs.add(q)
            elif board[q] == colour and q not in seen:
                seen.add(q)
                todo.append(q)
    return seen, libs


def play(board, nbrs, a, fault=None):
    """One ply of the mover (OWN) on the empty point a: (the board after it, the captured opp points, the board with the stone
    placed and nothing lifted).  Captures first, then suicide is executed."""
    after = list(board)
    after[a] = OWN
    placed = list(after)
    captured = set()

    def lift_own():
        pts, libs = chain(after, nbrs, a)
        if not libs:
            for p in pts:
                after[p] = EMPTY

    if fault == "capture_after_suicide":
        lift_own()
    for q in nbrs[a]:
        if after[q] == OPP:
            pts, libs = chain(after, nbrs, q)
            if not libs:
                captured |= pts
    for p in captured:
        after[p] = EMPTY
    if fault != "capture_after_suicide":
        lift_own()
    return after, captured, placed


def _bits(words):
    return [int(a) for a in np.flatnonzero(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little"))]


def read_record(S, rec, side=0, fault=None):
    """(board list over the area, prev point set or None, area, mover_white)"""
    N, NW = S * S, (S * S + 31) // 32
    p = np.asarray(rec, dtype=np.uint32).reshape(16, NW)
    flag = 32 * NW - 1
    wtp = bool(int(p[0, NW - 1]) >> 31)
    strip = fault in ("flag_as_stone", "padding_read")
    area = 32 * NW if strip else N
    keep = {"flag_as_stone": lambda a: a < N or a == flag, "padding_read": lambda a: a != flag}.get(fault, lambda a: a < N)
    keep_w = (lambda a: True) if fault == "padding_read" else (lambda a: a < N)
    black, white = [a for a in _bits(p[0]) if keep(a)], [a for a in _bits(p[1]) if keep_w(a)]
    mover_white = wtp != (side == 1)
    board = [EMPTY] * area
    for a in black:
        board[a] = OPP if mover_white else OWN
    for a in white:
        if board[a] == EMPTY:
            board[a] = OWN if mover_white else OPP
    has_prev = side == 0 or fault == "ko_at_side1"
    prev = None
    if has_prev:
        plane = 3 if mover_white else 2
        if fault == "ko_wrong_plane":
            plane = 5 - plane
        prev = {a for a in _bits(p[plane]) if a < N}
    return board, prev, area, mover_white


def ko_point(board, prev):
    """the point the one-stone ko approximation names, or -1"""
    if prev is None:
        return -1
    gone = [a for a in prev if board[a] != OWN]
    return gone[0] if len(gone) == 1 else -1


def record_moves(S, rec, side=0, fault=None):
    """(rows int16 [N, 8], counts int32 [8]) of one record"""
    N = S * S
    board, prev, area, _ = read_record(S, rec, side, fault)
    nbrs = neighbours(S, area)
    ko = ko_point(board, prev)
    rows = np.zeros((N, 8), np.int16)
    for a in range(N):
        flags = KO if a == ko else 0
        if board[a] != EMPTY:
            rows[a, 0] = flags | OCCUPIED
            continue
        after, captured, placed = play(board, nbrs, a, fault)
        suicide = after[a] == EMPTY
        size = libs = ataris = atari_stones = 0
        if not suicide:
            pts, lb = chain(after, nbrs, a)
            if fault == "libs_before_lift":
                lifted = list(after)
                for p in captured:
                    lifted[p] = OPP
                lb = chain(lifted, nbrs, a)[1]
            size, libs = len(pts), len(lb)
            seen = set()
            starts = [q for q in range(area) if after[q] == OPP] if fault == "ataris_anywhere" else [q for q in nbrs[a] if after[q] == OPP]
            for q in starts:
                if q in seen:
                    continue
                cp, cl = chain(after, nbrs, q)
                seen |= cp
                if len(cl) == 1:
                    ataris += 1
                    atari_stones += len(cp)
        if all(board[q] == EMPTY for q in nbrs[a]) and fault == "quiet_no_edge":
            libs = 4
        joined, weakest, seen = 0, 0, set()
        for q in nbrs[a]:
            if board[q] == OWN and (q not in seen or fault == "joined_stones"):
                cp, cl = chain(board, nbrs, q)
                seen |= cp
                L = len(cl) - (1 if fault == "weakest_without_a" else 0)
                weakest = L if joined == 0 else min(weakest, L)
                joined += 1
        if fault == "allowed_not_suicide":
            allowed = not suicide and a != ko
        else:
            allowed = (any(board[q] == EMPTY for q in nbrs[a]) or len(captured) > 0) and a != ko
        if allowed:
            flags |= ALLOWED
        if suicide:
            flags |= SUICIDE
        rows[a] = [flags, len(captured), size, libs, joined, weakest, ataris, atari_stones]
    return rows, counts_of(rows, fault)


def counts_of(rows, fault=None):
    """counts int32 [8] from the rows of one record, as the header states them"""
    r = rows.astype(np.int64)
    al = (r[:, 0] & ALLOWED) != 0
    c = np.zeros(8, np.int32)
    c[0] = al.sum()
    c[1] = (al & (r[:, 1] > 0)).sum()
    c[2] = r[al, 1].max() if al.any() else 0
    best = np.flatnonzero(al & (r[:, 1] == c[2])) if c[2] > 0 else []
    c[3] = -1 if c[2] == 0 else (best[-1] if fault == "max_move_highest" else best[0])
    c[4] = (al & (r[:, 3] == 1) & (r[:, 1] == 0)).sum()
    c[5] = (al & (r[:, 6] > 0)).sum()
    c[6] = (al & (r[:, 5] == 1) & (r[:, 3] >= 2)).sum()
    c[7] = ((r[:, 0] & (ALLOWED | OCCUPIED | KO | SUICIDE)) == 0).sum()
    return c


def moves(S, records, index=None, side=0, fault=None):
    """{"rows" int16 [n, N, 8], "counts" int32 [n, 8]}: one row per entry of index (None: every record); an index outside
    [0, R) gives zeros"""
    records = np.asarray(records)
    R = len(records)
    index = list(range(R)) if index is None else [int(i) for i in index]
    rows, counts = np.zeros((len(index), S * S, 8), np.int16), np.zeros((len(index), 8), np.int32)
    done = {}
    for i, r in enumerate(index):
        if 0 <= r < R:
            if r not in done:
                done[r] = record_moves(S, records[r], side, fault)
            rows[i], counts[i] = done[r]
    return {"rows": rows, "counts": counts}


def after_ply(S, rec, a, side=0):
    """(own points, opp points) of P' for the empty point a; for the comparison with oracle.make_play"""
    board, _, area, _ = read_record(S, rec, side)
    after = play(board, neighbours(S, area), a)[0]
    return [p for p in range(area) if after[p] == OWN], [p for p in range(area) if after[p] == OPP]
