"""CPU model of the capturing-race reader (include/sgo.h "capturing races"), written from the header's text: every ply is
oracle.make_play, ALLOWED / the pass / the root board are those of tests/solve_model.Reader (which stands on tests/tactics_model.py),
chains, liberties and regions are plain Python on integer bit sets (tactics_model.Sets).  No code of the package takes part.
Everything is integer: the GPU results must match word for word.

FAULT SWITCHES -- each the kind of slip the kernels could hold (tests/test_race_model_power.py shows which case notices which).
Model and test helper only; no library code reads them.
  desc_order             candidates are tried in descending order
  no_pass                the defender never passes
  no_wait                the attacker never waits: a ko ban with no other point of M left ends its moves
  no_second_order        M is M0 plus the inner chains: the second-order liberties are left out (the inner-chain test is against M0)
  no_inner_chains        the chains whose every liberty lies in M1 are not added to M
  outside_not_terminal   a liberty of the defender's racer outside M does not end the node SAFE
  cap_not_terminal       more than max_libs liberties do not end the node SAFE
  cap_off_by_one         the node ends SAFE at max_libs liberties already
  capture_not_terminal   the defender's capture of the stone on tA is not SAFE at once: the reader goes on below it
  adjacency_only         two chains are in contact only when their stones touch
  shared_miscount        word 4 counts lib(B) | lib(W) instead of lib(B) & lib(W)
  roles_exchanged        the black racer's answers stand in the white racer's words and bits, and the other way round
  shared_counter         the node counter is not restarted between A and D
  d_always               query D runs when A returned SAFE too
  outside_region         moves are not confined to M
  rules_ignored          rules = 1 is read as rules = 0
  no_root_ko             the ko test is ignored at the root
  ko_wrong_side          the ko `prev` is taken from the other side (the parent's own stones; at the root the other colour's plane)
  flag_as_stone          the to-play flag is read as a black stone.  INERT BY CONSTRUCTION: at every supported size the flag bit lies
                         at least one full padding row below the board (strip rows 6 / 9 / 10 / 14 / 20 at S = 5 / 7 / 9 / 13 / 19),
                         so a lone black stone there touches no board point: it forms no pair, and changes no liberty, region or
                         move of one.  tests/test_race_model_power.py shows that no case record changes under it
  padding_read           bits >= N of planes 0 / 1 (other than the flag) are read as stones

With flag_as_stone / padding_read the PAIR TABLE (chains, liberties, regions) is taken on the STRIP the plane words form (width S,
32 * NW points), as a kernel reading the words without a mask would see it; pairs with an anchor outside the board are listed and
not read, and the regions are reported for the points a < N."""
import numpy as np

from tests import solve_model as SM
from tests import tactics_model as T

FAULTS = ("desc_order", "no_pass", "no_wait", "no_second_order", "no_inner_chains", "outside_not_terminal", "cap_not_terminal",
          "cap_off_by_one", "capture_not_terminal", "adjacency_only", "shared_miscount", "roles_exchanged", "shared_counter", "d_always",
          "outside_region", "rules_ignored", "no_root_ko", "ko_wrong_side", "flag_as_stone", "padding_read")
SIZES = T.SIZES
MAX_LIBS, MAX_REGION, MAX_NODES, MAX_PAIRS, MAX_DEPTH = 8, 32, 32768, 64, 80
A_CAUGHT, D_CAUGHT, A_UNKNOWN, D_UNKNOWN, D_RAN = 1, 2, 4, 8, 16
WHITE_SHIFT = 8
OPEN, NO_PAIR = 1 << 16, 1 << 17
CAUGHT, SAFE, UNK = 1, 2, 3
NO_PAIR_ROW = [-1, -1, 0, 0, 0, 0, NO_PAIR, 0, -1, -1, -1, -1, 0, 0, 0, 0]
build_record = T.build_record
_words = SM._words


def _count(v):
    return bin(v).count("1")


def pair_table(S, rec, ask=None, region=None, max_libs=4, max_region=8, fault=None):
    """[(row words 0..7, the points of M)] of one record: enumerated (ask None) or the one asked row of ask = (p, q)"""
    N, NW = S * S, (S * S + 31) // 32
    p = T._planes(S, rec)
    black, white = [int(a) for a in T._bits(p[0])], [int(a) for a in T._bits(p[1])]
    flag = 32 * NW - 1
    keep_b = (lambda a: a != flag) if fault == "padding_read" else (lambda a: a < N or a == flag) if fault == "flag_as_stone" else \
        (lambda a: a < N)
    keep_w = (lambda a: a not in black) if fault == "padding_read" else (lambda a: a < N)
    black = [a for a in black if keep_b(a)]
    white = [a for a in white if keep_w(a)]
    area = 32 * NW if fault in ("padding_read", "flag_as_stone") else N
    g = T.Sets(S, area)
    b, w = g.of(black), g.of(white)
    emp = g.full & ~(b | w)

    def chains(stones):
        out, rest = [], stones
        while rest:
            c = g.flood(rest & -rest, rest)
            out.append(c)
            rest &= ~c
        return out

    def default_region(B, W):
        M0 = (g.nbr(B) | g.nbr(W)) & emp
        M1 = M0 if fault == "no_second_order" else M0 | (g.nbr(M0) & emp)
        M = M1
        if fault != "no_inner_chains":
            for c in chains(b & ~B) + chains(w & ~W):
                libs = g.nbr(c) & emp
                if libs and not libs & ~M1:
                    M |= c
        return M

    def head(B, W, M):
        lb, lw = g.nbr(B) & emp, g.nbr(W) & emp
        shared = _count(lb | lw) if fault == "shared_miscount" else _count(lb & lw)
        re = _count(M & emp)
        return [g.points(B)[0], g.points(W)[0], _count(lb), _count(lw), shared, re, 0 if 1 <= re <= max_region else OPEN, 0]

    if ask is not None:
        pq = [int(ask[0]), int(ask[1])]
        if any(a < 0 or a >= N or not (b | w) & g.bit(a) for a in pq) or bool(b & g.bit(pq[0])) == bool(b & g.bit(pq[1])):
            return [(NO_PAIR_ROW[:8], [])]
        pb, pw = pq if b & g.bit(pq[0]) else pq[::-1]
        B, W = g.flood(g.bit(pb), b), g.flood(g.bit(pw), w)
        if region is not None:
            M = g.of([int(a) for a in T._bits(np.asarray(region, np.uint32)) if a < N])
        else:
            M = default_region(B, W)
        return [(head(B, W, M), [a for a in g.points(M) if a < N])]
    out = []
    for B in chains(b):
        lb = g.nbr(B) & emp
        if not 1 <= _count(lb) <= max_libs:
            continue
        for W in chains(w):
            lw = g.nbr(W) & emp
            if not 1 <= _count(lw) <= max_libs:
                continue
            touch = bool(g.nbr(B) & W)
            if not touch and (fault == "adjacency_only" or not lb & lw):
                continue
            M = default_region(B, W)
            h = head(B, W, M)
            if h[6] == 0:
                out.append((h, [a for a in g.points(M) if a < N]))
    out.sort()
    return out


class Reader(SM.Reader):
    """The header's reader on one record.  deepest: the deepest node of the last query."""

    def __init__(self, S, rec, rules=1, max_libs=4, max_nodes=1024, fault=None, max_depth=MAX_DEPTH):
        SM.Reader.__init__(self, S, rec, rules, max_nodes, fault, max_depth)
        self.max_libs = max_libs

    def read(self, board, tD, tA, M, attacker_to_move, depth):
        """(CAUGHT | SAFE, the move that decided it or -1); raises T.Unknown.  M: a Sets value"""
        self.nodes += 1
        if self.nodes > self.max_nodes or depth > self.max_depth:
            raise T.Unknown()
        self.deepest = max(self.deepest, depth)
        N, g, fault = self.N, self.g, self.fault
        own, opp = self.sets_of(board)
        dst = opp if attacker_to_move else own
        emp = g.full & ~(own | opp)
        L = g.nbr(g.flood(g.bit(tD), dst)) & emp
        if L & ~M and fault != "outside_not_terminal":
            return SAFE, -1
        if fault != "cap_not_terminal" and _count(L) > self.max_libs - (1 if fault == "cap_off_by_one" else 0):
            return SAFE, -1
        ok = self.allowed(board)
        cands = [a for a in g.points(emp if fault == "outside_region" else emp & M) if ok[a]]
        if fault == "desc_order":
            cands.reverse()
        flat = board.reshape(N, 17)
        if attacker_to_move:
            for a in cands:
                child = self.play(board, a)
                cf = child.reshape(N, 17)                            # plane 0 the defender, plane 1 the attacker
                if not cf[tD, 0]:
                    return CAUGHT, a
                if not cf[a, 1]:
                    continue
                if self.read(child, tD, tA, M, False, depth + 1)[0] == CAUGHT:
                    return CAUGHT, a
            gone = np.flatnonzero((flat[:, 2] != 0) & (flat[:, 0] == 0))
            banned = len(gone) == 1 and bool(g.bit(int(gone[0])) & M & emp)
            if banned and fault != "no_wait" and self.read(self.passed(board), tD, tA, M, False, depth + 1)[0] == CAUGHT:
                return CAUGHT, N
            return SAFE, -1
        for a in cands:
            child = self.play(board, a)
            cf = child.reshape(N, 17)                                # plane 0 the attacker, plane 1 the defender
            if not cf[tD, 1] or not cf[a, 1]:
                continue
            if not cf[tA, 0] and fault != "capture_not_terminal":
                return SAFE, a
            if self.read(child, tD, tA, M, True, depth + 1)[0] == SAFE:
                return SAFE, a
        if fault != "no_pass" and self.read(self.passed(board), tD, tA, M, True, depth + 1)[0] == SAFE:
            return SAFE, N
        return CAUGHT, -1

    def query(self, tD, tA, colour, M, attacker_first, start_nodes=0):
        """(CAUGHT | SAFE | UNK, move, nodes counted); colour: the defender's"""
        self.nodes, self.deepest = start_nodes, 0
        mover = -colour if attacker_first else colour
        try:
            res, move = self.read(self.root_board(mover), tD, tA, M, attacker_first, 0)
        except T.Unknown:
            return UNK, -1, self.nodes
        return res, move, self.nodes

    def racer(self, tD, tA, colour, M):
        """(status bits, catch, save, nodes of A, nodes of D, [deepest of A, of D]) of one racer as the defender"""
        ra, ma, na = self.query(tD, tA, colour, M, True)
        depths = [self.deepest, 0]
        st = (A_CAUGHT if ra == CAUGHT else 0) | (A_UNKNOWN if ra == UNK else 0)
        catch, save, nd = (ma if ra == CAUGHT else -1), -1, 0
        if ra == CAUGHT or (self.fault == "d_always" and ra == SAFE):
            rd, md, nd = self.query(tD, tA, colour, M, False, na if self.fault == "shared_counter" else 0)
            depths[1] = self.deepest
            st |= D_RAN | (D_CAUGHT if rd == CAUGHT else 0) | (D_UNKNOWN if rd == UNK else 0)
            save = md if rd == SAFE else -1
        return st, catch, save, na, nd, depths

    def row(self, head, M):
        """the sixteen words of a table row from its first eight, and the deepest node of the four queries"""
        if head[6] or head[0] >= self.N or head[1] >= self.N:
            return list(head) + [-1, -1, -1, -1, 0, 0, 0, 0], [0, 0, 0, 0]
        Ms = self.g.of(M)
        bk = self.racer(head[0], head[1], 1, Ms)
        wh = self.racer(head[1], head[0], -1, Ms)
        if self.fault == "roles_exchanged":
            bk, wh = wh, bk
        row = list(head)
        row[6] |= bk[0] | (wh[0] << WHITE_SHIFT)
        return row + [bk[1], bk[2], wh[1], wh[2], bk[3], bk[4], wh[3], wh[4]], bk[5] + wh[5]


def record_race(S, rec, ask=None, region=None, rules=1, max_libs=4, max_region=8, max_nodes=1024, fault=None, max_depth=MAX_DEPTH):
    """(rows int32 [n_pairs, 16], regions uint32 [n_pairs, NW], depths int32 [n_pairs, 4]) of one record, every pair"""
    NW = (S * S + 31) // 32
    rd = Reader(S, rec, rules, max_libs, max_nodes, fault, max_depth)
    rows, regions, depths = [], [], []
    for head, M in pair_table(S, rec, ask, region, max_libs, max_region, fault):
        row, dd = rd.row(head, M)
        rows.append(row)
        regions.append(_words(M, NW))
        depths.append(dd)
    return np.array(rows, np.int32).reshape(-1, 16), np.array(regions, np.uint32).reshape(-1, NW), np.array(depths, np.int32).reshape(-1, 4)


def race(S, records, index=None, ask=None, region=None, rules=1, max_libs=4, max_region=8, max_nodes=1024, max_pairs=MAX_PAIRS, fault=None,
         max_depth=MAX_DEPTH):
    """The outputs of sgo_race_dev for n rows: {"n_pairs" int32 [n], "rows": a list of int32 [min(n_pairs, max_pairs), 16], "regions":
    the same of uint32 [.., NW], "depths": of int32 [.., 4]}.  records uint32 [R, 16 * NW]; index None = rows 0 .. R - 1; ask None or
    int [n, 2] (ask[i][0] < 0: enumerate); region None or uint32 [n, NW]; a row outside [0, R) gives n_pairs 0 and no rows."""
    records = np.asarray(records, dtype=np.uint32)
    R, NW = len(records), (S * S + 31) // 32
    index = np.arange(R) if index is None else np.asarray(index, dtype=np.int64)
    n = len(index)
    out = {"n_pairs": np.zeros(n, np.int32), "rows": [], "regions": [], "depths": []}
    cache = {}
    for i, r in enumerate(index):
        r = int(r)
        if r < 0 or r >= R:
            out["rows"].append(np.zeros((0, 16), np.int32))
            out["regions"].append(np.zeros((0, NW), np.uint32))
            out["depths"].append(np.zeros((0, 4), np.int32))
            continue
        a = None if ask is None or int(ask[i][0]) < 0 else (int(ask[i][0]), int(ask[i][1]))
        reg = None if region is None or a is None else np.asarray(region[i], np.uint32)
        key = (r, a, None if reg is None else reg.tobytes())
        if key not in cache:
            cache[key] = record_race(S, records[r], a, reg, rules, max_libs, max_region, max_nodes, fault, max_depth)
        rows, regions, depths = cache[key]
        out["n_pairs"][i] = len(rows)
        out["rows"].append(rows[:max_pairs])
        out["regions"].append(regions[:max_pairs])
        out["depths"].append(depths[:max_pairs])
    return out


def verdicts(row):
    """(black racer, white racer): `safe` / `unsettled` / `caught` / `unknown`, or `open` / `no_pair` for both"""
    st = int(row[6])
    if st & NO_PAIR:
        return "no_pair", "no_pair"
    if st & OPEN:
        return "open", "open"
    out = []
    for s in (st & 255, (st >> WHITE_SHIFT) & 255):
        out.append("unknown" if s & (A_UNKNOWN | D_UNKNOWN) else "safe" if not s & A_CAUGHT else "caught" if s & D_CAUGHT else "unsettled")
    return tuple(out)
