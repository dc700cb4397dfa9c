"""CPU model of the chains-and-ladders reader (include/sgo.h "chains and ladders"), written from the header's text: every ply is
oracle.make_play, every "allowed" is oracle.legal_moves on a board tensor whose plane 2 is `prev`; chains and liberties are plain
Python on integer bit sets.  No code of the package takes part.  Everything is integer: the GPU results must match word for word.

FAULT SWITCHES -- each the kind of slip the kernels could hold (tests/test_tactics_model_power.py shows which case notices
which).  Model and test helper only; no library code reads them.
  desc_order          liberties and candidates are tried in descending order
  no_counter          the defender's counter-captures are left out
  ko_wrong_side       the ko `prev` is taken from the other side (the parent's own stones; at the root the other colour's plane)
  no_root_ko          the ko test is ignored at the root
  root_ko_always      the root's ko test is applied even when the root's mover is not the record's side to move
  suicide_not_skipped the attacker's stone removed by suicide is not skipped.  INERT BY CONSTRUCTION: an allowed move has an empty
                      neighbour or captures, so its stone always keeps a liberty; no position can show this switch
  depth_off_by_one    the query ends unknown at depth >= MAX_DEPTH
  shared_counter      the node counter is not restarted between A and D
  libs_unsaturated    the liberty map is taken mod 256 instead of saturated (no chain of a 19x19 board has 255 liberties: shown on
                      saturate() alone)
  flag_as_stone       the to-play flag is read as a black stone
  padding_read        bits >= N of planes 0 / 1 (other than the flag) are read as stones
  anchor_highest      the anchor is the highest point of the chain

With flag_as_stone / padding_read the chain table is taken on the STRIP the plane words form (width S, 32 * NW points), as a
kernel reading the words without a mask would see it; chains anchored outside the board are listed and not read."""
import numpy as np

from oracle import oracle

FAULTS = ("desc_order", "no_counter", "ko_wrong_side", "no_root_ko", "root_ko_always", "suicide_not_skipped", "depth_off_by_one",
          "shared_counter", "libs_unsaturated", "flag_as_stone", "padding_read", "anchor_highest")
SIZES = (5, 7, 9, 13, 19)
MAX_CHAINS, MAX_NODES, MAX_DEPTH = 128, 512, 80
A_CAPTURED, D_CAPTURED, A_UNKNOWN, D_UNKNOWN, D_RAN = 1, 2, 4, 8, 16
CAP, ESC, UNK = 1, 2, 3


def saturate(n, fault=None):
    return n & 255 if fault == "libs_unsaturated" else min(255, n)


class Unknown(Exception):
    pass


# ---- integer bit sets: point a = y * S + x is bit y * (S + 1) + x, so that a shift never wraps into the next row ----------------
class Sets(object):
    def __init__(self, S, points):
        """points: how many points a < points belong to the area (N: the board; 32 * NW: the strip of the plane words)"""
        self.S, self.W = S, S + 1
        self.full = 0
        for a in range(points):
            self.full |= self.bit(a)

    def bit(self, a):
        return 1 << ((a // self.S) * self.W + a % self.S)

    def of(self, pts):
        v = 0
        for a in pts:
            v |= self.bit(a)
        return v

    def points(self, v):
        out = []
        while v:
            low = v & -v
            p = low.bit_length() - 1
            out.append((p // self.W) * self.S + p % self.W)
            v ^= low
        return out

    def nbr(self, v):
        return ((v << 1) | (v >> 1) | (v << self.W) | (v >> self.W)) & self.full

    def flood(self, seed, m):
        x = seed & m
        while True:
            t = (x | self.nbr(x)) & m
            if t == x:
                return x
            x = t


def _planes(S, rec):
    NW = (S * S + 31) // 32
    return np.asarray(rec, dtype=np.uint32).reshape(16, NW)


def _bits(words):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little"))


def record_sets(S, rec):
    """(black, white, black one ply ago, white one ply ago) as point lists a < N, and the to-play flag"""
    N, NW = S * S, (S * S + 31) // 32
    p = _planes(S, rec)
    sets = [[int(a) for a in _bits(p[k]) if a < N] for k in range(4)]
    return sets[0], sets[1], sets[2], sets[3], bool(p[0, NW - 1] >> 31)


def chain_table(S, rec, fault=None):
    """(libs uint8 [N], [[anchor, colour, size, liberties]] of the listed chains in ascending anchor order)"""
    N, NW = S * S, (S * S + 31) // 32
    p = _planes(S, rec)
    black, white = [int(a) for a in _bits(p[0])], [int(a) for a in _bits(p[1])]
    flag = 32 * NW - 1
    keep_b = (lambda a: a != flag) if fault == "padding_read" else (lambda a: a < N or a == flag) if fault == "flag_as_stone" else \
        (lambda a: a < N)
    keep_w = (lambda a: True) if fault == "padding_read" else (lambda a: a < N)
    black, white = [a for a in black if keep_b(a)], [a for a in white if keep_w(a)]
    g = Sets(S, 32 * NW if fault in ("padding_read", "flag_as_stone") else N)
    b, w = g.of(black), g.of(white)
    emp = g.full & ~(b | w)
    libs, rows = np.zeros(32 * NW, np.uint8), []
    for colour, stones in ((1, b), (-1, w)):
        rest = stones
        while rest:
            c = g.flood(rest & -rest, rest)
            pts = g.points(c)
            L = bin(g.nbr(c) & emp).count("1")
            libs[pts] = saturate(L, fault)
            if 1 <= L <= 2:
                rows.append([pts[-1] if fault == "anchor_highest" else pts[0], colour, len(pts), L])
            rest &= ~c
    rows.sort()
    return libs[:N].copy(), rows


class Reader(object):
    """The header's reader on one record.  stats: the deepest node and the node count of the last query."""

    def __init__(self, S, rec, fault=None, max_nodes=MAX_NODES, max_depth=MAX_DEPTH):
        self.S, self.N, self.fault = S, S * S, fault
        self.max_nodes, self.max_depth = max_nodes, max_depth
        self.g = Sets(S, self.N)
        self.black, self.white, self.pblack, self.pwhite, self.wtp = record_sets(S, rec)
        self.nodes, self.deepest = 0, 0

    def root_board(self, mover):
        """board tensor with `mover` (+1 / -1) to move: plane 0 its stones, plane 1 the other's, plane 2 its `prev`"""
        S, N = self.S, self.N
        own, opp = (self.black, self.white) if mover == 1 else (self.white, self.black)
        stm = -1 if self.wtp else 1
        restricted = mover == stm
        if self.fault == "no_root_ko":
            restricted = False
        if self.fault == "root_ko_always":
            restricted = True
        before = (self.pblack if mover == 1 else self.pwhite)
        if self.fault == "ko_wrong_side":
            before = (self.pwhite if mover == 1 else self.pblack)
        prev = before if restricted else own
        flat = np.zeros((N, 17), np.int32)
        flat[own, 0], flat[opp, 1], flat[prev, 2] = 1, 1, 1
        flat[:, 16] = mover
        return np.ascontiguousarray(flat.reshape(1, S, S, 17))

    def sets_of(self, board):
        N = self.N
        flat = board.reshape(N, 17)
        return self.g.of(np.flatnonzero(flat[:, 0]).tolist()), self.g.of(np.flatnonzero(flat[:, 1]).tolist())

    def play(self, board, a):
        child = board.copy()
        oracle.make_play(a % self.S, a // self.S, child)
        if self.fault == "ko_wrong_side":
            child[..., 2] = child[..., 3]
        return child

    def read(self, board, t, attacker_to_move, depth):
        """(CAP | ESC, the move that decided it or -1); raises Unknown"""
        self.nodes += 1
        over = depth >= self.max_depth if self.fault == "depth_off_by_one" else depth > self.max_depth
        if self.nodes > self.max_nodes or over:
            raise Unknown()
        self.deepest = max(self.deepest, depth)
        g, tb = self.g, self.g.bit(t)
        own, opp = self.sets_of(board)
        dst, ast = (opp, own) if attacker_to_move else (own, opp)
        emp = g.full & ~(own | opp)
        chain = g.flood(tb, dst)
        lib = g.nbr(chain) & emp
        L = bin(lib).count("1")
        illegal = oracle.legal_moves(board)
        rev = self.fault == "desc_order"
        if attacker_to_move:
            if L >= 3:
                return ESC, -1
            pts = sorted(g.points(lib), reverse=rev)
            if L == 1:
                return (CAP, pts[0]) if not illegal[pts[0]] else (ESC, -1)
            for a in pts:
                if illegal[a]:
                    continue
                child = self.play(board, a)
                cown, copp = self.sets_of(child)                 # the defender, the attacker
                if not cown & tb:
                    return CAP, a
                if not copp & g.bit(a) and self.fault != "suicide_not_skipped":
                    continue
                if self.read(child, t, False, depth + 1)[0] == CAP:
                    return CAP, a
            return ESC, -1
        cands = set(g.points(lib))
        if self.fault != "no_counter":
            rest = g.flood(g.nbr(chain) & ast, ast)
            while rest:
                c = g.flood(rest & -rest, rest)
                cl = g.nbr(c) & emp
                if bin(cl).count("1") == 1:
                    cands.update(g.points(cl))
                rest &= ~c
        for a in sorted(cands, reverse=rev):
            if illegal[a]:
                continue
            child = self.play(board, a)
            cown, copp = self.sets_of(child)                     # the attacker, the defender
            if not copp & tb:
                continue
            L2 = bin(g.nbr(g.flood(tb, copp)) & g.full & ~(cown | copp)).count("1")
            if L2 <= 1:
                continue
            if L2 >= 3:
                return ESC, a
            if self.read(child, t, True, depth + 1)[0] == ESC:
                return ESC, a
        return CAP, -1

    def query(self, t, colour, attacker_first, start_nodes=0):
        """(CAP | ESC | UNK, move, nodes counted)"""
        self.nodes, self.deepest = start_nodes, 0
        mover = -colour if attacker_first else colour
        try:
            res, move = self.read(self.root_board(mover), t, attacker_first, 0)
        except Unknown:
            return UNK, -1, self.nodes
        return res, move, self.nodes

    def chain_row(self, head):
        """the eight words of a chain row from its first four"""
        anchor, colour, size, L = head
        if anchor >= self.N:                                     # a chain the padding faults made up: listed, not read
            return [anchor, colour, size, L, 0, -1, -1, 0]
        self.depths = [0, 0]
        ra, ma, na = self.query(anchor, colour, True)
        self.depths[0] = self.deepest
        status = (A_CAPTURED if ra == CAP else 0) | (A_UNKNOWN if ra == UNK else 0)
        attack, defend, nodes = (ma if ra == CAP else -1), -1, na
        if L == 1 or (L == 2 and ra == CAP):
            rd, md, nd = self.query(anchor, colour, False, na if self.fault == "shared_counter" else 0)
            self.depths[1] = self.deepest
            status |= D_RAN | (D_CAPTURED if rd == CAP else 0) | (D_UNKNOWN if rd == UNK else 0)
            defend = md if rd == ESC else -1
            nodes += nd
        return [anchor, colour, size, L, status, attack, defend, nodes]


def record_tactics(S, rec, fault=None, max_nodes=MAX_NODES, max_depth=MAX_DEPTH):
    """(libs uint8 [N], rows int32 [n_chains, 8], depths int32 [n_chains, 2]: the deepest node of A and of D)"""
    libs, heads = chain_table(S, rec, fault)
    rd = Reader(S, rec, fault, max_nodes, max_depth)
    rows, depths = [], []
    for h in heads:
        rows.append(rd.chain_row(h))
        depths.append(list(getattr(rd, "depths", [0, 0])))
        rd.depths = [0, 0]
    return libs, np.array(rows, np.int32).reshape(-1, 8), np.array(depths, np.int32).reshape(-1, 2)


def tactics(S, records, index=None, max_chains=MAX_CHAINS, fault=None, max_nodes=MAX_NODES, max_depth=MAX_DEPTH):
    """The outputs of sgo_tactics_dev for n rows: {"libs" uint8 [n, N], "n_chains" int32 [n], "rows": a list of int32
    [min(n_chains, max_chains), 8], "depths": the same of [.., 2]}.  records uint32 [R, 16 * NW]; index None = rows 0 .. R - 1; a
    row outside [0, R) gives zero libs, n_chains 0 and no chain rows."""
    records = np.asarray(records, dtype=np.uint32)
    R, N = len(records), S * S
    index = np.arange(R) if index is None else np.asarray(index, dtype=np.int64)
    n = len(index)
    out = {"libs": np.zeros((n, N), np.uint8), "n_chains": np.zeros(n, np.int32), "rows": [], "depths": []}
    cache = {}
    for i, r in enumerate(index):
        r = int(r)
        if r < 0 or r >= R:
            out["rows"].append(np.zeros((0, 8), np.int32))
            out["depths"].append(np.zeros((0, 2), np.int32))
            continue
        if r not in cache:
            cache[r] = record_tactics(S, records[r], fault, max_nodes, max_depth)
        libs, rows, depths = cache[r]
        out["libs"][i], out["n_chains"][i] = libs, len(rows)
        out["rows"].append(rows[:max_chains])
        out["depths"].append(depths[:max_chains])
    return out


def build_record(S, black, white, white_to_play, prev_black=None, prev_white=None, rng=None):
    """uint32 [16 * NW]: planes 0 / 1 the stones, planes 2 / 3 the stones one ply ago (None: as now).  With rng: random words in
    planes 4..15 and in the padding bits of planes 0..3 (the flag is set as asked)."""
    N, NW = S * S, (S * S + 31) // 32
    rec = np.zeros((16, NW), np.uint32)
    if rng is not None:
        rec[:] = rng.randint(0, 1 << 32, size=(16, NW), dtype=np.uint64).astype(np.uint32)
        live = np.zeros(32 * NW, bool)
        live[:N] = True
        livew = np.packbits(live, bitorder="little").view("<u4").astype(np.uint32)
        rec[:4] &= ~livew
        rec[0, NW - 1] &= np.uint32(0x7fffffff)
    sets = (black, white, black if prev_black is None else prev_black, white if prev_white is None else prev_white)
    for plane, pts in enumerate(sets):
        for a in pts:
            rec[plane, a >> 5] |= np.uint32(1 << (a & 31))
    if white_to_play:
        rec[0, NW - 1] |= np.uint32(0x80000000)
    return rec.reshape(-1)
