"""CPU model of the connection reader (include/sgo.h "connections"), written from the header's text: every ply is oracle.make_play,
ALLOWED / the pass / the root board are those of tests/solve_model.Reader (which stands on tests/tactics_model.py), chains, liberties,
link points, regions and groups are plain Python on integer bit sets (tactics_model.Sets).  No code of the package takes part.
Everything is integer: the GPU results must match word for word.

FAULT SWITCHES -- each the kind of slip the kernels could hold (tests/test_connect_model_power.py shows which case notices which).
Model and test helper only; no library code reads them.
  desc_order             candidates are tried in descending order
  no_attacker_pass       the attacker never passes
  pass_only_ko           the attacker passes only while the ko test forbids it an empty point of M (the solve reader's wait)
  defender_passes        the defender tries a pass after its moves
  joined_wrong_anchor    the joined test floods from ty and looks for ty: it holds at once
  no_root_joined         the joined test is skipped at the root.  INERT BY CONSTRUCTION: a pair is two DIFFERENT chains at the root of
                         either query, so the test never holds there; tests/test_connect_model_power.py shows no case changes
  y_capture_not_cut      the attacker's capture of the stone on ty is not a cut at once (only that of tx is)
  common_libs_only       K is lib(X) & lib(Y): the liberties next to a liberty of the other chain are left out
  no_cutting_chains      cutting chains are ignored: their liberties do not join K, word 7 is 0
  cut_libs_off_by_one    a cutting chain may have cut_libs + 1 liberties
  cutting_not_in_m       a cutting chain is not added to M: the points it leaves when captured are not playable
  no_second_order        M1 is K alone
  no_inner_chains        the chains whose every liberty lies in M1 are not added to M
  anchors_unordered      an asked pair keeps the order it was asked in: anchor_x may be above anchor_y
  colours_mixed          an asked pair of two colours is read (the colour is that of the first stone) instead of NO_PAIR
  shared_counter         the node counter is not restarted between A and D
  d_always               query D runs when A returned JOINED too
  outside_region         moves are not confined to M
  rules_ignored          rules = 1 is read as rules = 0
  no_root_ko             the ko test is ignored at the root
  ko_wrong_side          the ko `prev` is taken from the other side (the parent's own stones; at the root the other colour's plane)
  padding_read           bits >= N of planes 0 / 1 (other than the flag) are read as stones
  groups_tie_unsettled   the group map ties `unsettled` pairs too
  groups_not_transitive  one sweep in descending row order without a fixed point: a label does not travel along a row of ties
  groups_across_colours  the map's chains are the 4-connected sets of stones of EITHER colour

With padding_read the PAIR TABLE (chains, liberties, regions) is taken on the STRIP the plane words form (width S, 32 * NW points), as a
kernel reading the words without a mask would see it; pairs with an anchor outside the board are listed and not read, and the regions
are reported for the points a < N."""
import numpy as np

from tests import solve_model as SM
from tests import tactics_model as T

FAULTS = ("desc_order", "no_attacker_pass", "pass_only_ko", "defender_passes", "joined_wrong_anchor", "no_root_joined", "y_capture_not_cut",
          "common_libs_only", "no_cutting_chains", "cut_libs_off_by_one", "cutting_not_in_m", "no_second_order", "no_inner_chains",
          "anchors_unordered", "colours_mixed", "shared_counter", "d_always", "outside_region", "rules_ignored", "no_root_ko", "ko_wrong_side",
          "padding_read", "groups_tie_unsettled", "groups_not_transitive", "groups_across_colours")
SIZES = T.SIZES
MAX_CUT_LIBS, MAX_REGION, MAX_NODES, MAX_PAIRS, MAX_DEPTH = 4, 32, 32768, 64, 80
A_CUT, D_CUT, A_UNKNOWN, D_UNKNOWN, D_RAN = 1, 2, 4, 8, 16
OPEN, NO_PAIR = 1 << 16, 1 << 17
CUT, JOINED, UNK = 1, 2, 3
W = 12                                                               # words of a table row
NO_PAIR_ROW = [-1, -1, 0, 0, 0, 0, NO_PAIR, 0, -1, -1, 0, 0]
FLAG_CUT_TABLE, FLAG_UNDECIDED = 1, 2
build_record = T.build_record
_words = SM._words


def _count(v):
    return bin(v).count("1")


def _sets(S, rec, fault):
    """(Sets, black, white) of a record: on the strip of the plane words under padding_read"""
    N, NW = S * S, (S * S + 31) // 32
    p = T._planes(S, rec)
    black, white = [int(a) for a in T._bits(p[0])], [int(a) for a in T._bits(p[1])]
    flag = 32 * NW - 1
    if fault == "padding_read":
        black = [a for a in black if a != flag]
        white = [a for a in white if a not in black]
    else:
        black, white = [a for a in black if a < N], [a for a in white if a < N]
    g = T.Sets(S, 32 * NW if fault == "padding_read" else N)
    return g, g.of(black), g.of(white)


def _chains(g, stones):
    out, rest = [], stones
    while rest:
        c = g.flood(rest & -rest, rest)
        out.append(c)
        rest &= ~c
    return out


def pair_table(S, rec, ask=None, region=None, cut_libs=1, max_region=8, fault=None):
    """[(row words 0..7, the points of M)] of one record: enumerated (ask None) or the one asked row of ask = (p, q)"""
    N = S * S
    g, b, w = _sets(S, rec, fault)
    emp = g.full & ~(b | w)
    limit = 0 if fault == "no_cutting_chains" else cut_libs + (1 if fault == "cut_libs_off_by_one" else 0)

    def head(X, Y, own, opp, given=None):
        lx, ly = g.nbr(X) & emp, g.nbr(Y) & emp
        K = lx & ly
        if fault != "common_libs_only":
            K |= (lx & g.nbr(ly)) | (ly & g.nbr(lx))
        cutting = []
        for Z in _chains(g, opp):
            if g.nbr(Z) & X and g.nbr(Z) & Y and 1 <= _count(g.nbr(Z) & emp) <= limit:
                cutting.append(Z)
                K |= g.nbr(Z) & emp
        M1 = K if fault == "no_second_order" else K | (g.nbr(K) & emp)
        M = M1
        for Z in cutting:
            if fault != "cutting_not_in_m":
                M |= Z
        if fault != "no_inner_chains":
            for c in _chains(g, own & ~(X | Y)) + [c for c in _chains(g, opp) if c not in cutting]:
                libs = g.nbr(c) & emp
                if libs and not libs & ~M1:
                    M |= c
        if given is not None:
            M = given
        re = _count(M & emp)
        colour = 1 if own == b else -1
        return [g.points(X)[0], g.points(Y)[0], colour, _count(lx & ly), _count(K), re, 0 if 1 <= re <= max_region else OPEN, len(cutting)], \
            [a for a in g.points(M) if a < N], K

    if ask is not None:
        p, q = int(ask[0]), int(ask[1])
        if any(a < 0 or a >= N or not (b | w) & g.bit(a) for a in (p, q)):
            return [(NO_PAIR_ROW[:8], [])]
        if bool(b & g.bit(p)) != bool(b & g.bit(q)) and fault != "colours_mixed":
            return [(NO_PAIR_ROW[:8], [])]
        own, opp = (b, w) if b & g.bit(p) else (w, b)
        X = g.flood(g.bit(p), own)
        Y = g.flood(g.bit(q), own if own & g.bit(q) else opp)
        if X == Y:
            return [(NO_PAIR_ROW[:8], [])]
        if g.points(X)[0] > g.points(Y)[0] and fault != "anchors_unordered":
            X, Y = Y, X
        given = None if region is None else g.of([int(a) for a in T._bits(np.asarray(region, np.uint32)) if a < N])
        h, M, K = head(X, Y, own, opp, given)
        return [(h, M)]
    out = []
    for own, opp in ((b, w), (w, b)):
        cs = _chains(g, own)
        for i, X in enumerate(cs):
            for Y in cs[i + 1:]:
                h, M, K = head(X, Y, own, opp)
                if K and h[6] == 0:
                    out.append((h, M))
    out.sort()
    return out


class Reader(SM.Reader):
    """The header's reader on one record.  deepest: the deepest node of the last query."""

    def __init__(self, S, rec, rules=1, max_nodes=1024, fault=None, max_depth=MAX_DEPTH):
        SM.Reader.__init__(self, S, rec, rules, max_nodes, fault, max_depth)

    def read(self, board, tx, ty, M, attacker_to_move, depth):
        """(CUT | JOINED, the move that decided it or -1); raises T.Unknown.  M: a Sets value"""
        self.nodes += 1
        if self.nodes > self.max_nodes or depth > self.max_depth:
            raise T.Unknown()
        self.deepest = max(self.deepest, depth)
        N, g, fault = self.N, self.g, self.fault
        own, opp = self.sets_of(board)
        dst = opp if attacker_to_move else own
        emp = g.full & ~(own | opp)
        if not (fault == "no_root_joined" and depth == 0):
            if g.flood(g.bit(ty if fault == "joined_wrong_anchor" else tx), dst) & g.bit(ty):
                return JOINED, -1
        ok = self.allowed(board)
        cands = [a for a in g.points(emp if fault == "outside_region" else emp & M) if ok[a]]
        if fault == "desc_order":
            cands.reverse()
        flat = board.reshape(N, 17)
        if attacker_to_move:
            for a in cands:
                child = self.play(board, a)
                cf = child.reshape(N, 17)                            # plane 0 the defender, plane 1 the attacker
                if not cf[tx, 0] or (not cf[ty, 0] and fault != "y_capture_not_cut"):
                    return CUT, a
                if not cf[a, 1]:
                    continue
                if self.read(child, tx, ty, M, False, depth + 1)[0] == CUT:
                    return CUT, a
            passes = fault != "no_attacker_pass"
            if fault == "pass_only_ko":
                gone = np.flatnonzero((flat[:, 2] != 0) & (flat[:, 0] == 0))
                passes = len(gone) == 1 and bool(g.bit(int(gone[0])) & M & emp)
            if passes and self.read(self.passed(board), tx, ty, M, False, depth + 1)[0] == CUT:
                return CUT, N
            return JOINED, -1
        for a in cands:
            child = self.play(board, a)
            cf = child.reshape(N, 17)                                # plane 0 the attacker, plane 1 the defender
            if not cf[tx, 1] or not cf[ty, 1] or not cf[a, 1]:
                continue
            if self.read(child, tx, ty, M, True, depth + 1)[0] == JOINED:
                return JOINED, a
        if fault == "defender_passes" and self.read(self.passed(board), tx, ty, M, True, depth + 1)[0] == JOINED:
            return JOINED, N
        return CUT, -1

    def query(self, tx, ty, colour, M, attacker_first, start_nodes=0):
        """(CUT | JOINED | UNK, move, nodes counted); colour: the defender's"""
        self.nodes, self.deepest = start_nodes, 0
        mover = -colour if attacker_first else colour
        try:
            res, move = self.read(self.root_board(mover), tx, ty, M, attacker_first, 0)
        except T.Unknown:
            return UNK, -1, self.nodes
        return res, move, self.nodes

    def row(self, head, M):
        """the twelve words of a table row from its first eight, and the deepest node of A and of D"""
        if head[6] or head[0] >= self.N or head[1] >= self.N:
            return list(head) + [-1, -1, 0, 0], [0, 0]
        Ms = self.g.of(M)
        tx, ty, colour = head[0], head[1], head[2]
        ra, ma, na = self.query(tx, ty, colour, Ms, True)
        depths = [self.deepest, 0]
        st = (A_CUT if ra == CUT else 0) | (A_UNKNOWN if ra == UNK else 0)
        cut, join, nd = (ma if ra == CUT else -1), -1, 0
        if ra == CUT or (self.fault == "d_always" and ra == JOINED):
            rd, md, nd = self.query(tx, ty, colour, Ms, False, na if self.fault == "shared_counter" else 0)
            depths[1] = self.deepest
            st |= D_RAN | (D_CUT if rd == CUT else 0) | (D_UNKNOWN if rd == UNK else 0)
            join = md if rd == JOINED else -1
        row = list(head)
        row[6] |= st
        return row + [cut, join, na, nd], depths


def verdict(row):
    """`connected` / `unsettled` / `cut` / `unknown` / `open` / `no_pair` of a table row"""
    st = int(row[6])
    if st & NO_PAIR:
        return "no_pair"
    if st & OPEN:
        return "open"
    if st & (A_UNKNOWN | D_UNKNOWN):
        return "unknown"
    if not st & A_CUT:
        return "connected"
    return "cut" if st & D_CUT else "unsettled"


def group_map(S, rec, rows, n_pairs, fault=None):
    """(groups int16 [N], counts int32 [4]) of one record from its WRITTEN table rows and the true pair count"""
    N = S * S
    g, b, w = _sets(S, rec, fault)
    chains = _chains(g, b | w) if fault == "groups_across_colours" else _chains(g, b) + _chains(g, w)
    label = {}
    for c in chains:
        a = g.points(c)[0]
        for pt in g.points(c):
            label[pt] = a                                            # a stone names its chain's anchor; the anchor its label
    lab = {g.points(c)[0]: g.points(c)[0] for c in chains}
    ties, flags, connected = [], FLAG_CUT_TABLE if n_pairs > len(rows) else 0, 0
    for row in rows:
        v = verdict(row)
        if v in ("unknown", "open"):
            flags |= FLAG_UNDECIDED
        if v == "connected":
            connected += 1
        if v == "connected" or (v == "unsettled" and fault == "groups_tie_unsettled"):
            ties.append((label.get(int(row[0]), int(row[0])), label.get(int(row[1]), int(row[1]))))
    if fault == "groups_not_transitive":
        for x, y in reversed(ties):
            lab[x] = lab[y] = min(lab[x], lab[y])
    else:
        changed = True
        while changed:
            changed = False
            for x, y in ties:
                m = min(lab[x], lab[y])
                if lab[x] != m or lab[y] != m:
                    lab[x] = lab[y] = m
                    changed = True
    out = np.full(N, -1, np.int16)
    for pt, a in label.items():
        if pt < N:
            out[pt] = lab[a]
    return out, np.array([len(chains), sum(1 for a in lab if lab[a] == a), connected, flags], np.int32)


def record_connect(S, rec, ask=None, region=None, rules=1, cut_libs=1, max_region=8, max_nodes=1024, fault=None, max_depth=MAX_DEPTH):
    """(rows int32 [n_pairs, 12], regions uint32 [n_pairs, NW], depths int32 [n_pairs, 2]) of one record, every pair"""
    NW = (S * S + 31) // 32
    rd = Reader(S, rec, rules, max_nodes, fault, max_depth)
    rows, regions, depths = [], [], []
    for head, M in pair_table(S, rec, ask, region, cut_libs, max_region, fault):
        row, dd = rd.row(head, M)
        rows.append(row)
        regions.append(_words(M, NW))
        depths.append(dd)
    return np.array(rows, np.int32).reshape(-1, W), np.array(regions, np.uint32).reshape(-1, NW), np.array(depths, np.int32).reshape(-1, 2)


def connect(S, records, index=None, ask=None, region=None, rules=1, cut_libs=1, max_region=8, max_nodes=1024, max_pairs=MAX_PAIRS, fault=None,
            max_depth=MAX_DEPTH):
    """The outputs of sgo_connect_dev for n rows: {"n_pairs" int32 [n], "rows": a list of int32 [min(n_pairs, max_pairs), 12], "regions":
    the same of uint32 [.., NW], "depths": of int32 [.., 2], "groups": a list of int16 [N] (None: untouched), "counts": of int32 [4]
    (None: untouched)}.  records uint32 [R, 16 * NW]; index None = rows 0 .. R - 1; ask None or int [n, 2] (ask[i][0] < 0: enumerate);
    region None or uint32 [n, NW]; a row outside [0, R) gives n_pairs 0, no rows and an untouched map."""
    records = np.asarray(records, dtype=np.uint32)
    R, NW = len(records), (S * S + 31) // 32
    index = np.arange(R) if index is None else np.asarray(index, dtype=np.int64)
    n = len(index)
    out = {"n_pairs": np.zeros(n, np.int32), "rows": [], "regions": [], "depths": [], "groups": [], "counts": []}
    cache = {}
    for i, r in enumerate(index):
        r = int(r)
        if r < 0 or r >= R:
            out["rows"].append(np.zeros((0, W), np.int32))
            out["regions"].append(np.zeros((0, NW), np.uint32))
            out["depths"].append(np.zeros((0, 2), np.int32))
            out["groups"].append(None)
            out["counts"].append(None)
            continue
        a = None if ask is None or int(ask[i][0]) < 0 else (int(ask[i][0]), int(ask[i][1]))
        reg = None if region is None or a is None else np.asarray(region[i], np.uint32)
        key = (r, a, None if reg is None else reg.tobytes())
        if key not in cache:
            rows, regions, depths = record_connect(S, records[r], a, reg, rules, cut_libs, max_region, max_nodes, fault, max_depth)
            cache[key] = (rows, regions, depths) + group_map(S, records[r], rows[:max_pairs], len(rows), fault)
        rows, regions, depths, groups, counts = cache[key]
        out["n_pairs"][i] = len(rows)
        out["rows"].append(rows[:max_pairs])
        out["regions"].append(regions[:max_pairs])
        out["depths"].append(depths[:max_pairs])
        out["groups"].append(groups)
        out["counts"].append(counts)
    return out
