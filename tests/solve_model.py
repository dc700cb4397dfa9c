"""CPU model of the life-and-death reader (include/sgo.h "life and death"), written from the header's text: every ply is
oracle.make_play, every ALLOWED of rules = 0 is oracle.legal_moves on a board tensor whose plane 2 is `prev` (the board plumbing is
tests/tactics_model.Reader's), alive_X is tests/life_model.benson, the "stone would stand" test of rules = 1 is the ply of
tests/moves_model.py; chains and regions are plain Python on integer bit sets.  No code of the package takes part.  Everything is
integer: the GPU results must match word for word.

FAULT SWITCHES -- each the kind of slip the kernels could hold (tests/test_solve_model_power.py shows which case notices which).
Model and test helper only; no library code reads them.
  desc_order             candidates are tried in descending order
  pass_first             the defender's pass is tried before its moves
  no_pass                the defender never passes
  attacker_passes        the attacker tries a pass after its moves whether or not a ko ban is in force
  no_wait                the attacker never waits: a ko ban with no other point of M left ends its moves
  no_inner_chains        the attacker chains whose every liberty lies in R are not added to M
  alive_root_only        the ALIVE test is made at the root only
  alive_attacker_colour  the ALIVE test runs unconditional life on the attacker's colour (the target is never in that set)
  ko_wrong_side          the ko `prev` is taken from the other side (the parent's own stones; at the root the other colour's plane)
  no_root_ko             the ko test is ignored at the root
  root_ko_always         the root's ko test is applied even when the root's mover is not the record's side to move
  depth_off_by_one       the query ends unknown at depth >= MAX_DEPTH
  shared_counter         the node counter is not restarted between A and D
  d_always               query D runs when A returned ALIVE too
  outside_region         moves are not confined to M
  rules_ignored          rules = 1 is read as rules = 0
  flag_as_stone          the to-play flag is read as a black stone
  padding_read           bits >= N of planes 0 / 1 (other than the flag) are read as stones

With flag_as_stone / padding_read the TARGET TABLE (chains, alive sets, regions) is taken on the STRIP the plane words form (width
S, 32 * NW points), as a kernel reading the words without a mask would see it; chains anchored outside the board are listed and not
read, and the regions are reported for the points a < N."""
import numpy as np

from oracle import oracle
from tests import life_model as LM
from tests import moves_model as MM
from tests import tactics_model as T

FAULTS = ("desc_order", "pass_first", "no_pass", "attacker_passes", "no_wait", "no_inner_chains", "alive_root_only", "alive_attacker_colour",
          "ko_wrong_side", "no_root_ko", "root_ko_always", "depth_off_by_one", "shared_counter", "d_always", "outside_region",
          "rules_ignored", "flag_as_stone", "padding_read")
SIZES = T.SIZES
MAX_REGION, MAX_NODES, MAX_TARGETS, MAX_DEPTH = 32, 65536, 64, 80
A_DEAD, D_DEAD, A_UNKNOWN, D_UNKNOWN, D_RAN, OPEN, NO_STONE = 1, 2, 4, 8, 16, 32, 64
DEAD, ALIVE, UNK = 1, 2, 3
build_record = T.build_record


def _words(pts, NW):
    w = np.zeros(NW, np.uint32)
    for a in pts:
        w[a >> 5] |= np.uint32(1 << (a & 31))
    return w


def target_table(S, rec, ask=-1, region=None, max_region=12, fault=None):
    """[(row words 0..3, the points of M)] of one record: enumerated (ask < 0) or the one asked row"""
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
    alive = g.of(LM.benson(S, black, white, None, area)[0]) | g.of(LM.benson(S, white, black, None, area)[0])

    def default_region(c, O):
        R = g.flood(c, g.full & ~O)
        M, rest = R, O
        while rest and fault != "no_inner_chains":
            ch = g.flood(rest & -rest, rest)
            libs = g.nbr(ch) & emp
            if libs and not libs & ~R:
                M |= ch
            rest &= ~ch
        return M

    if ask >= 0:
        if ask >= N or not (b | w) & g.bit(ask):
            return [([-1, 0, 0, NO_STONE], [])]
        colour = 1 if b & g.bit(ask) else -1
        X, O = (b, w) if colour == 1 else (w, b)
        c = g.flood(g.bit(ask), X)
        if region is not None:
            M = g.of([int(a) for a in T._bits(np.asarray(region, np.uint32)) if a < N])
        else:
            M = default_region(c, O)
        re = bin(M & emp).count("1")
        return [([g.points(c)[0], colour, re, 0 if 1 <= re <= max_region else OPEN], [a for a in g.points(M) if a < N])]
    out = []
    for colour, X, O in ((1, b, w), (-1, w, b)):
        rest = X
        while rest:
            c = g.flood(rest & -rest, rest)
            rest &= ~c
            if c & alive:
                continue
            M = default_region(c, O)
            re = bin(M & emp).count("1")
            if 1 <= re <= max_region:
                out.append(([g.points(c)[0], colour, re, 0], [a for a in g.points(M) if a < N]))
    out.sort()
    return out


class Reader(T.Reader):
    """The header's reader on one record.  deepest: the deepest node of the last query."""

    def __init__(self, S, rec, rules=1, max_nodes=4096, fault=None, max_depth=MAX_DEPTH):
        T.Reader.__init__(self, S, rec, fault, max_nodes, max_depth)
        self.rules = 0 if fault == "rules_ignored" else rules
        self.nbrs = MM.neighbours(S, self.N)
        self._alive = {}

    def alive(self, own, opp):
        """alive_X of the position, X = `own` (point tuples); positions repeat in a search without a table, so the sets are kept"""
        key = (own, opp)
        if key not in self._alive:
            self._alive[key] = LM.benson(self.S, own, opp)[0]
        return self._alive[key]

    def allowed(self, board):
        """the ALLOWED points a < N of the board's mover"""
        N = self.N
        flat = board.reshape(N, 17)
        ok = [not v for v in oracle.legal_moves(board)[:N]]
        if self.rules == 1:
            own, opp, prev = flat[:, 0], flat[:, 1], flat[:, 2]
            gone = np.flatnonzero((prev != 0) & (own == 0))
            ko = int(gone[0]) if len(gone) == 1 else -1
            cells = [MM.OWN if own[a] else MM.OPP if opp[a] else MM.EMPTY for a in range(N)]
            for a in range(N):
                if not ok[a] and cells[a] == MM.EMPTY and a != ko and MM.play(cells, self.nbrs, a)[0][a] == MM.OWN:
                    ok[a] = True
        return ok

    def passed(self, board):
        """the board after a pass of its mover: the same stones, and the new mover's `prev` is what it holds"""
        child = np.zeros_like(board)
        child[..., 0], child[..., 1], child[..., 16] = board[..., 1], board[..., 0], -board[..., 16]
        child[..., 2] = board[..., 0] if self.fault == "ko_wrong_side" else board[..., 1]
        return child

    def read(self, board, t, M, attacker_to_move, depth):
        """(DEAD | ALIVE, the move that decided it or -1); raises T.Unknown"""
        self.nodes += 1
        over = depth >= self.max_depth if self.fault == "depth_off_by_one" else depth > self.max_depth
        if self.nodes > self.max_nodes or over:
            raise T.Unknown()
        self.deepest = max(self.deepest, depth)
        N, fault = self.N, self.fault
        flat = board.reshape(N, 17)
        own, opp = tuple(np.flatnonzero(flat[:, 0]).tolist()), tuple(np.flatnonzero(flat[:, 1]).tolist())
        dst, ast = (opp, own) if attacker_to_move else (own, opp)
        if fault != "alive_root_only" or depth == 0:
            if t in (self.alive(ast, dst) if fault == "alive_attacker_colour" else self.alive(dst, ast)):
                return ALIVE, -1
        ok = self.allowed(board)
        stones = set(own) | set(opp)
        cands = [a for a in range(N) if (a in M or fault == "outside_region") and a not in stones and ok[a]]
        if fault == "desc_order":
            cands.reverse()
        if attacker_to_move:
            for a in cands:
                child = self.play(board, a)
                cf = child.reshape(N, 17)                            # plane 0 the defender, plane 1 the attacker
                if not cf[t, 0]:
                    return DEAD, a
                if not cf[a, 1]:
                    continue
                if self.read(child, t, M, False, depth + 1)[0] == DEAD:
                    return DEAD, a
            # the WAIT: only while the ko test forbids the attacker an empty point of M
            gone = np.flatnonzero((flat[:, 2] != 0) & (flat[:, 0] == 0))
            banned = len(gone) == 1 and int(gone[0]) in M and int(gone[0]) not in stones
            if fault == "no_wait":
                banned = False
            if (banned or fault == "attacker_passes") and self.read(self.passed(board), t, M, False, depth + 1)[0] == DEAD:
                return DEAD, N
            return ALIVE, -1
        if fault == "pass_first" and self.read(self.passed(board), t, M, True, depth + 1)[0] == ALIVE:
            return ALIVE, N
        for a in cands:
            child = self.play(board, a)
            cf = child.reshape(N, 17)                                # plane 0 the attacker, plane 1 the defender
            if not cf[t, 1] or not cf[a, 1]:
                continue
            if self.read(child, t, M, True, depth + 1)[0] == ALIVE:
                return ALIVE, a
        if fault not in ("pass_first", "no_pass") and self.read(self.passed(board), t, M, True, depth + 1)[0] == ALIVE:
            return ALIVE, N
        return DEAD, -1

    def query(self, t, colour, M, attacker_first, start_nodes=0):
        """(DEAD | ALIVE | UNK, move, nodes counted)"""
        self.nodes, self.deepest = start_nodes, 0
        mover = -colour if attacker_first else colour
        try:
            res, move = self.read(self.root_board(mover), t, M, attacker_first, 0)
        except T.Unknown:
            return UNK, -1, self.nodes
        return res, move, self.nodes

    def row(self, head, M):
        """the eight words of a table row from its first four, and the deepest node of A and of D"""
        anchor, colour, re, status = head
        if status or anchor >= self.N:
            return [anchor, colour, re, status, -1, -1, 0, 0], [0, 0]
        M = set(M)
        ra, ma, na = self.query(anchor, colour, M, True)
        depths = [self.deepest, 0]
        status = (A_DEAD if ra == DEAD else 0) | (A_UNKNOWN if ra == UNK else 0)
        kill, live, nd = (ma if ra == DEAD else -1), -1, 0
        if ra == DEAD or (self.fault == "d_always" and ra == ALIVE):
            rd, md, cnt = self.query(anchor, colour, M, False, na if self.fault == "shared_counter" else 0)
            depths[1] = self.deepest
            status |= D_RAN | (D_DEAD if rd == DEAD else 0) | (D_UNKNOWN if rd == UNK else 0)
            live, nd = (md if rd == ALIVE else -1), cnt
        return [anchor, colour, re, status, kill, live, na, nd], depths


def record_solve(S, rec, ask=-1, region=None, rules=1, max_region=12, max_nodes=4096, fault=None, max_depth=MAX_DEPTH):
    """(rows int32 [n_targets, 8], regions uint32 [n_targets, NW], depths int32 [n_targets, 2]) of one record, every target"""
    NW = (S * S + 31) // 32
    rd = Reader(S, rec, rules, max_nodes, fault, max_depth)
    rows, regions, depths = [], [], []
    for head, M in target_table(S, rec, ask, region, max_region, fault):
        row, dd = rd.row(head, M)
        rows.append(row)
        regions.append(_words(M, NW))
        depths.append(dd)
    return np.array(rows, np.int32).reshape(-1, 8), np.array(regions, np.uint32).reshape(-1, NW), np.array(depths, np.int32).reshape(-1, 2)


def solve(S, records, index=None, ask=None, region=None, rules=1, max_region=12, max_nodes=4096, max_targets=MAX_TARGETS, fault=None,
          max_depth=MAX_DEPTH):
    """The outputs of sgo_solve_dev for n rows: {"n_targets" int32 [n], "rows": a list of int32 [min(n_targets, max_targets), 8],
    "regions": the same of uint32 [.., NW], "depths": of int32 [.., 2]}.  records uint32 [R, 16 * NW]; index None = rows 0 .. R - 1;
    ask None or int [n] (< 0: enumerate); region None or uint32 [n, NW]; a row outside [0, R) gives n_targets 0 and no rows."""
    records = np.asarray(records, dtype=np.uint32)
    R, NW = len(records), (S * S + 31) // 32
    index = np.arange(R) if index is None else np.asarray(index, dtype=np.int64)
    n = len(index)
    out = {"n_targets": np.zeros(n, np.int32), "rows": [], "regions": [], "depths": []}
    cache = {}
    for i, r in enumerate(index):
        r = int(r)
        if r < 0 or r >= R:
            out["rows"].append(np.zeros((0, 8), np.int32))
            out["regions"].append(np.zeros((0, NW), np.uint32))
            out["depths"].append(np.zeros((0, 2), np.int32))
            continue
        a = -1 if ask is None else int(ask[i])
        reg = None if region is None or a < 0 else np.asarray(region[i], np.uint32)
        key = (r, a if a >= 0 else -1, None if reg is None else reg.tobytes())
        if key not in cache:
            cache[key] = record_solve(S, records[r], a, reg, rules, max_region, max_nodes, fault, max_depth)
        rows, regions, depths = cache[key]
        out["n_targets"][i] = len(rows)
        out["rows"].append(rows[:max_targets])
        out["regions"].append(regions[:max_targets])
        out["depths"].append(depths[:max_targets])
    return out
