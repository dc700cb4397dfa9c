"""CPU model of the securing-move table (include/sgo.h "securing moves"), written from the header's text on plain Python sets of
points: its own ply (place the stone, lift the opponent's chains without a liberty, then the mover's own), ALLOWED from the header's
words (an empty neighbour or a capture, and never the ko point), and unconditional life from tests/life_model.benson, which
tests/test_life_model_power.py pins.  No bitboards, and no code of the package takes part; tests/test_secure_model_power.py ties
the positions after the ply to oracle.make_play, the ALLOWED bits to oracle.legal_moves and the table to life_model.point_life.
Everything is integer: the GPU results must match word for word.

FAULT SWITCHES -- each the kind of slip a kernel could hold (tests/test_secure_model_power.py shows which case notices which).
Model and test helper only; no library code reads them.
  captures_kept           life is read with the captured stones still on the board
  stone_not_placed        life is read without the new stone (the captures are taken)
  base_for_every_point    every empty point carries the life of the position itself: the ply is forgotten
  opponent_benson         the wrong colour's life: alive / terr of the opponent in P'
  dead_from_before        `dead` counts the opp stones of the record inside terr, the captured ones too
  suicide_kept            a suicide is not executed: the stone and its chain stay for the life reading
  summary_over_all_empty  counts 3..7 run over every empty point, ALLOWED or not
  ko_on_side1             `prev` (the mover's plane) and the ko test are applied at side 1 as well
  best_highest_on_tie     best_move is the highest point that reaches best_gain
  best_sets_of_base       sets 2 / 3 repeat the life of the position itself
  gain_alive_only         gain is taken from alive alone (counts 4, 5, 6, 7)
  flag_as_stone           the to-play flag is read as a black stone

With flag_as_stone the position is taken on the STRIP the plane words form (width S, 32 * NW points), as a kernel reading the words
without a mask would see it; table rows are reported for the points a < N only."""
import functools

import numpy as np

from tests import life_model as L

FAULTS = ("captures_kept", "stone_not_placed", "base_for_every_point", "opponent_benson", "dead_from_before", "suicide_kept",
          "summary_over_all_empty", "ko_on_side1", "best_highest_on_tie", "best_sets_of_base", "gain_alive_only", "flag_as_stone")
SIZES = L.SIZES
ALLOWED, OCCUPIED, KO, SUICIDE = 1, 2, 4, 8
COUNTS = ("base_alive", "base_terr", "base_dead", "allowed", "securing", "best_gain", "best_move", "harmful")


def read_record(S, rec, side=0, fault=None):
    """(own, opp, prev or None, area): the mover's stones, the other colour's, the mover's stones one ply ago (side 0 only), and
    how many points the position has"""
    N, NW = S * S, (S * S + 31) // 32
    p = np.asarray(rec, dtype=np.uint32).reshape(16, NW)
    flag = 32 * NW - 1
    white_to_play = bool(int(p[0, NW - 1]) >> 31)
    area = 32 * NW if fault == "flag_as_stone" else N
    black = {a for a in L.points_of(p[0], 32 * NW) if a < N or (fault == "flag_as_stone" and a == flag)}
    white = {a for a in L.points_of(p[1], N)} - black
    mover_white = white_to_play != (side == 1)
    own, opp = (white, black) if mover_white else (black, white)
    prev = None
    if side == 0 or fault == "ko_on_side1":
        prev = set(L.points_of(p[3 if mover_white else 2], N))
    return own, opp, prev, area


def chain(S, stones, a, area):
    """the chain of `stones` on a, as a set"""
    seen, todo = {a}, [a]
    while todo:
        for b in L.neighbours(S, todo.pop(), area):
            if b in stones and b not in seen:
                seen.add(b)
                todo.append(b)
    return seen


def liberties(S, pts, own, opp, area):
    return {b for a in pts for b in L.neighbours(S, a, area) if b not in own and b not in opp}


def ply(S, own, opp, a, area):
    """One ply of the mover on the empty point a: (own', opp', captured).  Captures first, then suicide is executed."""
    own2, opp2, captured = set(own) | {a}, set(opp), set()
    for b in L.neighbours(S, a, area):
        if b in opp2:
            c = chain(S, opp2, b, area)
            if not liberties(S, c, own2, opp2, area):
                captured |= c
                opp2 -= c
    c = chain(S, own2, a, area)
    if not liberties(S, c, own2, opp2, area):
        own2 -= c
    return own2, opp2, captured


def ko_point(own, prev):
    """the point the one-stone ko approximation names, or -1"""
    if prev is None:
        return -1
    gone = [a for a in prev if a not in own]
    return gone[0] if len(gone) == 1 else -1


@functools.lru_cache(maxsize=64)
def position_secure(S, own, opp, area, fault=None):
    """What depends on the stones alone (own / opp frozensets), shared by the records that hold the same stones for the same mover:
    (alive, terr of the position, {empty a: (stone stands, captured any, alive, terr, dead) of P'})"""
    def life(o, p):
        al, te, _ = L.benson(S, p, o, area=area) if fault == "opponent_benson" else L.benson(S, o, p, area=area)
        return frozenset(al), frozenset(te)

    after = {}
    for a in range(S * S):
        if a in own or a in opp:
            continue
        own2, opp2, captured = ply(S, own, opp, a, area)
        o, p = set(own2), set(opp2)
        if fault == "captures_kept":
            p = set(opp)
        if fault == "stone_not_placed":
            o.discard(a)
        if fault == "suicide_kept" and a not in own2:
            o = set(own) | {a}
        if fault == "base_for_every_point":
            o, p = own, opp
        al, te = life(o, p)
        after[a] = (a in own2, bool(captured), al, te, len(te & (opp if fault == "dead_from_before" else p)))
    return life(own, opp) + (after,)


def record_secure(S, rec, side=0, fault=None):
    """(table int16 [N, 4], sets uint32 [4, NW], counts int32 [8]) of one record"""
    N, NW = S * S, (S * S + 31) // 32
    own, opp, prev, area = read_record(S, rec, side, fault)
    ko = ko_point(own, prev)
    base_alive, base_terr, after = position_secure(S, frozenset(own), frozenset(opp), area, fault)
    table = np.zeros((N, 4), np.int16)
    for a in range(N):
        flags = KO if a == ko else 0
        if a in own or a in opp:
            table[a, 0] = flags | OCCUPIED
            continue
        stands, captured, al, te, dead = after[a]
        if not stands:
            flags |= SUICIDE
        if (any(b not in own and b not in opp for b in L.neighbours(S, a, area)) or captured) and a != ko:
            flags |= ALLOWED
        table[a] = [flags, len(al), len(te), dead]
    t = table.astype(np.int64)
    base = len(base_alive) + len(base_terr)
    if fault == "gain_alive_only":
        gain = t[:, 1] - len(base_alive)
    else:
        gain = t[:, 1] + t[:, 2] - base
    sel = (t[:, 0] & ALLOWED) != 0
    if fault == "summary_over_all_empty":
        sel = (t[:, 0] & OCCUPIED) == 0
    counts = np.zeros(8, np.int32)
    counts[0], counts[1], counts[2] = len(base_alive), len(base_terr), len(base_terr & opp)
    counts[3] = sel.sum()
    counts[4] = (sel & (gain > 0)).sum()
    counts[7] = (sel & (gain < 0)).sum()
    best = -1
    if sel.any():
        counts[5] = gain[sel].max()
        reach = np.flatnonzero(sel & (gain == counts[5]))
        best = int(reach[-1] if fault == "best_highest_on_tie" else reach[0])
    counts[6] = best
    star = after[best][2:4] if best >= 0 and fault != "best_sets_of_base" else (base_alive, base_terr)
    sets = np.stack([L._words(base_alive, NW), L._words(base_terr, NW), L._words(star[0], NW), L._words(star[1], NW)])
    return table, sets, counts


def secure(S, records, index=None, side=0, fault=None):
    """The outputs of sgo_secure_dev for n rows: {"table" int16 [n, N, 4], "sets" uint32 [n, 4, NW], "counts" int32 [n, 8]}: one
    row per entry of index (None: every record); an index outside [0, R) gives zeros"""
    records = np.asarray(records)
    R, NW = len(records), (S * S + 31) // 32
    index = list(range(R)) if index is None else [int(i) for i in index]
    n = len(index)
    out = {"table": np.zeros((n, S * S, 4), np.int16), "sets": np.zeros((n, 4, NW), np.uint32), "counts": np.zeros((n, 8), np.int32)}
    done = {}
    for i, r in enumerate(index):
        if 0 <= r < R:
            if r not in done:
                done[r] = record_secure(S, records[r], side, fault)
            out["table"][i], out["sets"][i], out["counts"][i] = done[r]
    return out


def after_ply(S, rec, a, side=0):
    """(own points, opp points) of P' for the empty point a; for the comparison with oracle.make_play"""
    own, opp, _, area = read_record(S, rec, side)
    own2, opp2, _ = ply(S, own, opp, a, area)
    return sorted(own2), sorted(opp2)


def gains(out, i):
    """int [N]: alive + terr - base of every point of row i (meaningless on an occupied point)"""
    t, c = out["table"][i].astype(np.int64), out["counts"][i]
    return t[:, 1] + t[:, 2] - int(c[0]) - int(c[1])
