"""CPU model of the superko analysis (include/sgo.h "superko"), written from the header's text.  It stands on tests/moves_model.py
for the record reader, the ply (captures first, then suicide executed) and the legal set's rule; a position is a pair of Python
integers, one bit per stone, and two positions are compared by comparing those integers -- the STONES, never a key.  No code of the
package takes part.  Everything is integer: the GPU results must match word for word (counts[6], the refuted key matches, is the
kernel's own business and is 0 here).

FAULT SWITCHES -- each the kind of slip the kernel could hold (tests/test_superko_model_power.py shows that the case set notices
every one).  Model and test helper only; no library code reads them.
  history_without_r   the history leaves out r: a single-stone suicide no longer repeats
  history_before_f    the history reaches f - 1, the last record of the game before
  history_past_r      the history reaches r + 1
  smallest_h          the smallest matching h is taken instead of the largest
  flag_swapped        the to-play flag is ignored under rule 1 and used under rule 0
  quiet_skipped       points without a stone among their neighbours are not looked at
  captures_stay       the captured stones are left on the board of P'
  no_suicide          suicide is not executed: the stones without a liberty stay in P'
  extra_unmasked      `extra` is not masked by the legal set
  seen_at_r           `seen` may match h = r (and is then 0 plies back, which hides every earlier match)"""
import numpy as np

from tests import moves_model as M

FAULTS = ("history_without_r", "history_before_f", "history_past_r", "smallest_h", "flag_swapped", "quiet_skipped", "captures_stay",
          "no_suicide", "extra_unmasked", "seen_at_r")
SIZES = M.SIZES
COUNTS = ("repeat", "extra", "max_back", "max_back_point", "seen", "history", "refuted", "truncated")


def max_history(S):
    return 4 * S * S + 1                       # SGO_SUPERKO_MAX_HISTORY


def position(S, rec):
    """(black, white, white_to_play) of a record: the stones as integers with bit a for point a"""
    board, _, _, mover_white = M.read_record(S, rec)
    own = sum(1 << a for a, v in enumerate(board) if v == M.OWN)
    opp = sum(1 << a for a, v in enumerate(board) if v == M.OPP)
    return (opp, own, True) if mover_white else (own, opp, False)


def _plies(S, rec, fault=None):
    """[(a, black', white', legal)] for every empty point a of the record, ascending: the stones of P' and whether the record's own
    legal set holds a"""
    board, prev, area, mover_white = M.read_record(S, rec)
    nbrs = M.neighbours(S, area)
    ko = M.ko_point(board, prev)
    own = sum(1 << a for a, v in enumerate(board) if v == M.OWN)
    opp = sum(1 << a for a, v in enumerate(board) if v == M.OPP)
    out = []
    for a in range(S * S):
        if board[a] != M.EMPTY:
            continue
        quiet = all(board[q] == M.EMPTY for q in nbrs[a])
        if quiet and fault == "quiet_skipped":
            continue
        after, captured, _ = M.play(board, nbrs, a)
        o2, p2 = own | (1 << a), opp
        if fault != "captures_stay":
            for p in captured:
                p2 &= ~(1 << p)
        if after[a] == M.EMPTY and fault != "no_suicide":
            o2 = sum(1 << p for p, v in enumerate(after) if v == M.OWN)
        legal = (any(board[q] == M.EMPTY for q in nbrs[a]) or len(captured) > 0) and a != ko
        out.append((a, p2 if mover_white else o2, o2 if mover_white else p2, legal))
    return out, mover_white


def superko(S, records, rows, rule=0, fault=None):
    """{"sets" uint32 [n, 3, NW], "back" int16 [n, N], "counts" int32 [n, 8]} for rows [(r, f)] over records [R, 16 * NW]"""
    records = np.asarray(records)
    R, N, NW = len(records), S * S, (S * S + 31) // 32
    n = len(rows)
    bits = np.zeros((n, 3, 32 * NW), np.uint8)
    back = np.full((n, N), -1, np.int16)
    counts = np.zeros((n, 8), np.int32)
    pos, plies = {}, {}

    def P(h):
        if h not in pos:
            pos[h] = position(S, records[h])
        return pos[h]

    use_flag = (rule == 1) != (fault == "flag_swapped")
    for i, (r, f) in enumerate(rows):
        r, f = int(r), int(f)
        if not (0 <= r < R and 0 <= f <= r):
            continue
        span = r - f + 1
        nh = min(span, max_history(S))
        lo = r - nh + 1
        first = max(lo - 1, 0) if fault == "history_before_f" else lo
        last = r - 1 if fault == "history_without_r" else (min(r + 1, R - 1) if fault == "history_past_r" else r)
        where = {}                                                   # position -> the h that wins
        for h in range(first, last + 1):
            b, w, t = P(h)
            key = (b, w, t) if use_flag else (b, w)
            if fault != "smallest_h" or key not in where:
                where[key] = h
        if r not in plies:
            plies[r] = _plies(S, records[r], fault)
        cand, mover_white = plies[r]
        best, best_pt = 0, -1
        for a, b2, w2, legal in cand:
            key = (b2, w2, not mover_white) if use_flag else (b2, w2)
            if key not in where:
                continue
            k = r - where[key]
            back[i, a] = k
            bits[i, 0, a] = 1
            if legal or fault == "extra_unmasked":
                bits[i, 1, a] = 1
                if best_pt < 0 or k > best:
                    best, best_pt = k, a
        for a, _, _, legal in cand:
            if legal and not bits[i, 0, a]:
                bits[i, 2, a] = 1
        if fault == "quiet_skipped":                                 # the points the fault never looked at are still legal
            board, prev, area, _ = M.read_record(S, records[r])
            nbrs, ko = M.neighbours(S, area), M.ko_point(board, prev)
            for a in range(N):
                if board[a] == M.EMPTY and all(board[q] == M.EMPTY for q in nbrs[a]) and nbrs[a] and a != ko:
                    bits[i, 2, a] = 1
        bits[i, 2, N] = 1                                            # the pass
        b, w, t = P(r)
        key = (b, w, t) if use_flag else (b, w)
        seen = 0
        top = r if fault == "seen_at_r" else r - 1
        for h in range(min(top, last), first - 1, -1):
            bh, wh, th = P(h)
            if ((bh, wh, th) if use_flag else (bh, wh)) == key:
                seen = r - h
                break
        counts[i] = [bits[i, 0].sum(), bits[i, 1].sum(), best, best_pt, seen, nh, 0, 1 if span > max_history(S) else 0]
    sets = np.packbits(bits, axis=2, bitorder="little").view("<u4").astype(np.uint32).reshape(n, 3, NW)
    return {"sets": sets, "back": back, "counts": counts}


def after_position(S, rec, a):
    """(black, white, white_to_play) after one ply of the side to move on the empty point a, as integers: for building cases"""
    cand, mover_white = _plies(S, rec)
    for p, b2, w2, _ in cand:
        if p == a:
            return b2, w2, not mover_white
    raise ValueError("point %d is not empty" % a)
