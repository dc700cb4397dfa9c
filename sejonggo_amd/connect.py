"""Connections on the device (include/sgo.h "connections", csrc/sgo_connect.hip): per position the pairs of two chains of one colour
that are near each other (or the one pair asked for), the region M each pair is read in, whether an exhaustive reader bounded by M
lets the other colour cut them apart -- moving first (`cut_move`) and even moving second -- and the map of the GROUPS the `connected`
pairs tie the chains into.  A bounded reader, not a proof about the game: no transposition table, the one-ply ko approximation, no
move outside M, no capture of a cutting chain with more than cut_libs liberties, and `connected` says one chain, not a living one.

    from sejonggo_amd.connect import connect
    v = connect(19, records)                     # packed records uint32 [R, 16 * NW], host or device; every near pair
    for p in v.pairs_of(0): print(p.anchor_x, p.anchor_y, p.verdict, p.cut_move, p.join_move)
    v.groups[0]                                  # int16 [N]: per stone the lowest anchor of its group, -1 on empty points
    v = connect(19, records, ask=[(72, 74)])     # the chains on points 72 and 74 of record 0, in their default region

records.RecordSet.connect() reads every position of a game collection, engine.SessionEngine.connect(slots) the positions of session
slots; GTP's `sgo-connect` and `sgo-groups`, `python -m sejonggo_amd.review --connect` and `python -m sejonggo_amd.records --connect`
stand on them."""
import collections
import ctypes as C

import numpy as np

from ._packed import device_records, points as _points

A_CUT, D_CUT, A_UNKNOWN, D_UNKNOWN, D_RAN = 1, 2, 4, 8, 16
OPEN, NO_PAIR = 1 << 16, 1 << 17
MAX_CUT_LIBS, MAX_REGION, MAX_NODES, MAX_PAIRS = 4, 32, 32768, 64
WORDS = 12
VERDICTS = ("connected", "unsettled", "cut", "unknown", "open")
FLAG_CUT_TABLE, FLAG_UNDECIDED = 1, 2


def verdict_of(status):
    """the word of a table row from its status: `connected` (A JOINED), `unsettled` (A CUT, D JOINED), `cut` (both CUT), `unknown` (a
    query ran out of its budget), `open` (no query ran: the region is empty or too large), `no pair`"""
    status = int(status)
    if status & NO_PAIR:
        return "no pair"
    if status & OPEN:
        return "open"
    if status & (A_UNKNOWN | D_UNKNOWN):
        return "unknown"
    if not status & A_CUT:
        return "connected"
    return "cut" if status & D_CUT else "unsettled"


_FIELDS = "anchor_x anchor_y colour shared links region_empty status cutting cut_move join_move nodes_a nodes_d"


class Pair(collections.namedtuple("Pair", _FIELDS)):
    """One row of the pair table.  cut_move / join_move -1: none; cut_move N: the attacker's pass (it cuts by playing elsewhere)."""
    __slots__ = ()

    @property
    def open(self):
        return bool(self.status & OPEN)

    @property
    def no_pair(self):
        return bool(self.status & NO_PAIR)

    @property
    def verdict(self):
        return verdict_of(self.status)


def check_args(rules, cut_libs, max_region, max_nodes, max_pairs):
    if rules not in (0, 1):
        raise ValueError("rules must be 0 (inherited) or 1 (sound)")
    if not 0 <= int(cut_libs) <= MAX_CUT_LIBS:
        raise ValueError("cut_libs must be in [0, %d]" % MAX_CUT_LIBS)
    if not 1 <= int(max_region) <= MAX_REGION:
        raise ValueError("max_region must be in [1, %d]" % MAX_REGION)
    if not 1 <= int(max_nodes) <= MAX_NODES:
        raise ValueError("max_nodes must be in [1, %d]" % MAX_NODES)
    if not 1 <= int(max_pairs) <= MAX_PAIRS:
        raise ValueError("max_pairs must be in [1, %d]" % MAX_PAIRS)


class Connect(object):
    """n_pairs int32 [n] (the true number), rows int32 [n, max_pairs, 12], regions uint32 [n, max_pairs, NW] (the first
    min(n_pairs, max_pairs) of each position), groups int16 [n, N], group_counts int32 [n, 4] = chains, groups, connected pairs, flags."""

    def __init__(self, size, n_pairs, rows, regions, groups, group_counts, status=None):
        self.S, self.N = size, size * size
        self.n_pairs, self.rows = np.asarray(n_pairs, dtype=np.int32), np.asarray(rows, dtype=np.int32)
        self.regions = np.asarray(regions, dtype=np.uint32)
        self.groups, self.group_counts = np.asarray(groups, dtype=np.int16), np.asarray(group_counts, dtype=np.int32)
        self.status = status

    def __len__(self):
        return len(self.n_pairs)

    def listed(self, i):
        return min(int(self.n_pairs[i]), self.rows.shape[1])

    def pairs_of(self, i):
        return [Pair(*(int(v) for v in row)) for row in self.rows[i, :self.listed(i)]]

    def verdicts(self, i):
        """the verdict words of the listed pairs of row i"""
        return [p.verdict for p in self.pairs_of(i)]

    def region(self, i, k):
        """the points of M of pair k of row i"""
        return _points(self.regions[i, k], self.N)

    def find(self, i, anchor_x, anchor_y):
        """the Pair of row i with those anchors, or None"""
        for p in self.pairs_of(i):
            if (p.anchor_x, p.anchor_y) == (anchor_x, anchor_y):
                return p
        return None

    def groups_of(self, i):
        """{group label (its lowest anchor): the sorted points of its stones} of row i"""
        out = {}
        for a, g in enumerate(self.groups[i].tolist()):
            if g >= 0:
                out.setdefault(g, []).append(a)
        return out


def connect_dev(size, records, idx, ask, region, rules, cut_libs, max_region, max_nodes, max_pairs, lib):
    """sgo_connect_dev on device tensors: (n_pairs int32 [n], rows int32 [n, max_pairs, 12], regions int32 [n, max_pairs, NW], groups
    int16 [n, N] preset to -1, group_counts int32 [n, 4]) on the device; idx None: every record in order; ask / region None or device
    tensors int32 [n, 2] / [n, NW]"""
    import torch
    from . import _lib
    check_args(rules, cut_libs, max_region, max_nodes, max_pairs)
    R = int(records.shape[0])
    n = R if idx is None else int(idx.shape[0])
    dev = records.device
    n_pairs = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = torch.zeros((n, int(max_pairs), WORDS), dtype=torch.int32, device=dev)
    regions = torch.zeros((n, int(max_pairs), lib.sgo_plane_words(size)), dtype=torch.int32, device=dev)
    groups = torch.full((n, size * size), -1, dtype=torch.int16, device=dev)
    counts = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    _lib.check(lib.sgo_connect_dev(C.c_int(size), C.c_int(n), _lib.ptr(records), C.c_int(R), _lib.ptr(idx), _lib.ptr(ask), _lib.ptr(region),
                                   C.c_int(int(rules)), C.c_int(int(cut_libs)), C.c_int(int(max_region)), C.c_int(int(max_nodes)),
                                   C.c_int(int(max_pairs)), _lib.ptr(n_pairs), _lib.ptr(rows), _lib.ptr(regions), _lib.ptr(groups),
                                   _lib.ptr(counts), _lib.stream_ptr()), "sgo_connect_dev")
    return n_pairs, rows, regions, groups, counts


def host_inputs(size, n, ask, region):
    """(ask int32 [n, 2] or None, region uint32 [n, NW] or None) as contiguous host arrays, checked"""
    from .race import host_inputs as pair_inputs
    return pair_inputs(size, n, ask, region)


def connect(size, records, index=None, ask=None, region=None, rules=1, cut_libs=1, max_region=8, max_nodes=1024, max_pairs=MAX_PAIRS):
    """sgo_connect_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Connect with one row per
    entry of `index` (None: every record in order); an index outside [0, R) gives n_pairs 0 and a map of -1.  ask None: every near
    pair of every row; else two points per row ((-1, -1): enumerate that row), read in row i of `region` (uint32 [n, NW]) when given."""
    import torch
    from . import _lib
    check_args(rules, cut_libs, max_region, max_nodes, max_pairs)
    records, _, idx, n = device_records(size, records, index)
    ask, region = host_inputs(size, n, ask, region)
    d_ask = None if ask is None else torch.from_numpy(ask).to(records.device)
    d_region = None if region is None else torch.from_numpy(region.view(np.int32)).to(records.device)
    out = connect_dev(size, records, idx, d_ask, d_region, rules, cut_libs, max_region, max_nodes, max_pairs, _lib.load())
    n_pairs, rows, regions, groups, counts = (t.cpu().numpy() for t in out)
    return Connect(size, n_pairs, rows, regions.view(np.uint32), groups, counts)


def format_pair(p, vertex, N):
    """`sgo-connect` line of a Pair: `D4 F4 black shared 1 links 1 empty 3 cutting 0 unsettled cut E4 join E4 nodes 8 10`"""
    move = lambda a: "none" if a < 0 else "pass" if a >= N else vertex(a)                # noqa: E731
    if p.no_pair:
        return "no pair"
    return "%s %s %s shared %d links %d empty %d cutting %d %s cut %s join %s nodes %d %d" % (
        vertex(p.anchor_x), vertex(p.anchor_y), "black" if p.colour > 0 else "white", p.shared, p.links, p.region_empty, p.cutting, p.verdict,
        move(p.cut_move), move(p.join_move), p.nodes_a, p.nodes_d)


def format_groups(size, groups, black):
    """`sgo-groups` picture of one map (int16 [N]; `black`: the set of black points): one letter per group in ascending label order,
    upper case for black groups and lower case for white ones (the letters repeat past 25 groups of a colour), `.` for empty points;
    row S at the top as GTP's showboard draws it"""
    groups = [int(g) for g in groups]
    names, used = {}, {True: 0, False: 0}
    for g in sorted(set(v for v in groups if v >= 0)):
        is_b = g in black
        ch = "ABCDEFGHJKLMNOPQRSTUVWXYZ"[used[is_b] % 25]
        names[g] = ch if is_b else ch.lower()
        used[is_b] += 1
    lines = []
    for y in range(size):
        lines.append("%2d %s" % (size - y, " ".join(names.get(groups[y * size + x], ".") for x in range(size))))
    lines.append("   " + " ".join("ABCDEFGHJKLMNOPQRST"[:size]))
    return "\n".join(lines)


# ---- game review: was the played move the cut or the join of an unsettled pair? -------------------------------------------------
def deciding_moves(pairs, colour, N):
    """({point: anchor_x of the pair it cuts}, {point: anchor_x of the pair it joins}) of the side `colour` (+1 black, -1 white) from
    the Pair list of a position: its cut_move of every unsettled pair of the OTHER colour, its join_move of every unsettled pair of
    its own; passes are left out.  Where two pairs name one point the first listed stays."""
    cuts, joins = {}, {}
    for p in pairs:
        if p.verdict != "unsettled":
            continue
        if p.colour == colour and 0 <= p.join_move < N:
            joins.setdefault(p.join_move, p.anchor_x)
        if p.colour == -colour and 0 <= p.cut_move < N:
            cuts.setdefault(p.cut_move, p.anchor_x)
    return cuts, joins


def review_flags(size, action, colour, before, vertex=str):
    """Flags of one move by `colour` from the Pair list of the position in front of it:
      `cuts V`              the move is the cut_move of an unsettled pair (anchor V) of the opponent;
      `joins V`             the move is the join_move of an unsettled pair of the mover;
      `missed-cut V at K`, `missed-join V at K`   such a move K existed and another was played (one flag per pair anchor; none of a
                            kind when the move made one of that kind).
    These are flags from a bounded reader, not verdicts: unknown and open rows are never flagged."""
    cuts, joins = deciding_moves(before, colour, size * size)
    flags = []
    for word, moves in (("cut", cuts), ("join", joins)):
        if action in moves:
            flags.append("%ss %s" % (word, vertex(moves[action])))
            continue
        seen = set()
        for k in sorted(moves):
            if moves[k] not in seen:
                seen.add(moves[k])
                flags.append("missed-%s %s at %s" % (word, vertex(moves[k]), vertex(k)))
    return flags


# ---- record statistics: pairs per position, verdict shares, groups beside chains ------------------------------------------------
def bucket_table(ply, rows, n_pairs, group_counts, width=20):
    """The table of `records --connect` from one entry per position: ply int [n] (0-based move number), rows int32 [n, P, 12], n_pairs
    int [n], group_counts int [n, 4].  A list of dicts per bucket of `width` plies in ascending order: {"from", "to", "plies", "pairs"
    (listed rows), "found" (the true pair counts), "connected", "unsettled", "cut", "unknown", "open" (listed rows of each verdict),
    "chains", "groups" (summed over the positions), "cut_tables" (positions with flag 1)}."""
    ply, rows, n_pairs = np.asarray(ply, np.int64), np.asarray(rows, np.int64), np.asarray(n_pairs, np.int64)
    gc = np.asarray(group_counts, np.int64).reshape(-1, 4)
    listed = np.arange(rows.shape[1])[None, :] < np.minimum(n_pairs, rows.shape[1])[:, None]
    st = rows[:, :, 6]
    read = listed & ((st & (OPEN | NO_PAIR)) == 0)
    unk = (st & (A_UNKNOWN | D_UNKNOWN)) != 0
    words = {"open": listed & ((st & OPEN) != 0), "unknown": read & unk, "connected": read & ~unk & ((st & A_CUT) == 0),
             "unsettled": read & ~unk & ((st & A_CUT) != 0) & ((st & D_CUT) == 0), "cut": read & ~unk & ((st & A_CUT) != 0) & ((st & D_CUT) != 0)}
    out = []
    for b in sorted(set((ply // width).tolist())):
        sel = (ply // width) == b
        r = {"from": int(b * width + 1), "to": int((b + 1) * width), "plies": int(sel.sum()), "pairs": int(listed[sel].sum()),
             "found": int(n_pairs[sel].sum()), "chains": int(gc[sel, 0].sum()), "groups": int(gc[sel, 1].sum()),
             "cut_tables": int((gc[sel, 3] & FLAG_CUT_TABLE != 0).sum())}
        for v in VERDICTS:
            r[v] = int(words[v][sel].sum())
        out.append(r)
    return out


def format_bucket_table(table):
    lines = ["moves      plies  pairs/ply  connected  unsettled    cut  unknown   open  chains/ply  groups/ply"]
    for r in table:
        n, p = max(1, r["pairs"]), max(1, r["plies"])
        lines.append("%4d-%-4d  %5d  %9.2f  %8.0f%%  %8.0f%%  %4.0f%%  %6.0f%%  %4.0f%%  %10.2f  %10.2f" % (
            r["from"], r["to"], r["plies"], r["pairs"] / p, 100.0 * r["connected"] / n, 100.0 * r["unsettled"] / n, 100.0 * r["cut"] / n,
            100.0 * r["unknown"] / n, 100.0 * r["open"] / n, r["chains"] / p, r["groups"] / p))
    return "\n".join(lines)
