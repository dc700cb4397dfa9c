"""Capturing races on the device (include/sgo.h "capturing races", csrc/sgo_race.hip): per position the pairs of a black and a white
chain that lean on each other short of liberties (or the one pair asked for), the region M each pair is read in, and for EACH of the
two chains whether an exhaustive reader bounded by M catches it -- with the other side moving first (`catch`) and even with its own
side moving first -- while the other chain can be captured back.  A bounded reader, not a proof about the game: no transposition
table, the one-ply ko approximation, no snapback under a captured racer, no move outside M, and a verdict about two chains, not
their groups.

    from sejonggo_amd.race import race
    v = race(19, records)                        # packed records uint32 [R, 16 * NW], host or device; every pair in contact
    for p in v.pairs_of(0): print(p.anchor_b, p.anchor_w, p.black, p.white, p.outcome, p.catch_b, p.save_b, p.catch_w, p.save_w)
    v = race(19, records, ask=[(72, 73)])        # the chains on points 72 and 73 of record 0, in their default region
    v.region(0, 0)                               # the points of M

records.RecordSet.race() reads every position of a game collection, engine.SessionEngine.race(slots) the positions of session
slots; GTP's `sgo-race`, `python -m sejonggo_amd.review --race` and `python -m sejonggo_amd.records --race` stand on them."""
import collections
import ctypes as C

import numpy as np

from ._packed import device_records, points as _points

A_CAUGHT, D_CAUGHT, A_UNKNOWN, D_UNKNOWN, D_RAN = 1, 2, 4, 8, 16
WHITE_SHIFT = 8
OPEN, NO_PAIR = 1 << 16, 1 << 17
MAX_LIBS, MAX_REGION, MAX_NODES, MAX_PAIRS = 8, 32, 32768, 64
VERDICTS = ("safe", "unsettled", "caught", "unknown")


def verdict_of(bits):
    """the word of one racer from its five status bits: `safe` (A not CAUGHT), `unsettled` (A CAUGHT, D not), `caught` (both),
    `unknown` (a query ran out of its budget)"""
    bits = int(bits)
    if bits & (A_UNKNOWN | D_UNKNOWN):
        return "unknown"
    if not bits & A_CAUGHT:
        return "safe"
    return "caught" if bits & D_CAUGHT else "unsettled"


_FIELDS = "anchor_b anchor_w libs_b libs_w shared region_empty status reserved catch_b save_b catch_w save_w nodes_ab nodes_db nodes_aw nodes_dw"


class Pair(collections.namedtuple("Pair", _FIELDS)):
    """One row of the pair table.  catch_x / save_x -1: none; save_x N: the pass; catch_x N: the attacker's wait."""
    __slots__ = ()

    @property
    def open(self):
        return bool(self.status & OPEN)

    @property
    def no_pair(self):
        return bool(self.status & NO_PAIR)

    @property
    def black(self):
        """the black racer's word, None for an open row or one without a pair"""
        return None if self.status & (OPEN | NO_PAIR) else verdict_of(self.status & 255)

    @property
    def white(self):
        return None if self.status & (OPEN | NO_PAIR) else verdict_of((self.status >> WHITE_SHIFT) & 255)

    @property
    def outcome(self):
        """the pair in words: `black wins` (black safe, white caught), `white wins`, `first to move wins` (both unsettled), `standoff`
        (both safe: a seki, or neither can approach); otherwise the two racer words (`black safe, white unsettled`); `open` /
        `no pair` where no query ran"""
        if self.no_pair:
            return "no pair"
        if self.open:
            return "open"
        b, w = self.black, self.white
        if (b, w) == ("safe", "caught"):
            return "black wins"
        if (b, w) == ("caught", "safe"):
            return "white wins"
        if (b, w) == ("unsettled", "unsettled"):
            return "first to move wins"
        if (b, w) == ("safe", "safe"):
            return "standoff"
        return "black %s, white %s" % (b, w)


def check_args(rules, max_libs, max_region, max_nodes, max_pairs):
    if rules not in (0, 1):
        raise ValueError("rules must be 0 (inherited) or 1 (sound)")
    if not 1 <= int(max_libs) <= MAX_LIBS:
        raise ValueError("max_libs must be in [1, %d]" % MAX_LIBS)
    if not 1 <= int(max_region) <= MAX_REGION:
        raise ValueError("max_region must be in [1, %d]" % MAX_REGION)
    if not 1 <= int(max_nodes) <= MAX_NODES:
        raise ValueError("max_nodes must be in [1, %d]" % MAX_NODES)
    if not 1 <= int(max_pairs) <= MAX_PAIRS:
        raise ValueError("max_pairs must be in [1, %d]" % MAX_PAIRS)


class Race(object):
    """n_pairs int32 [n] (the true number), rows int32 [n, max_pairs, 16], regions uint32 [n, max_pairs, NW] (the first
    min(n_pairs, max_pairs) of each position)."""

    def __init__(self, size, n_pairs, rows, regions, status=None):
        self.S, self.N = size, size * size
        self.n_pairs, self.rows = np.asarray(n_pairs, dtype=np.int32), np.asarray(rows, dtype=np.int32)
        self.regions = np.asarray(regions, dtype=np.uint32)
        self.status = status

    def __len__(self):
        return len(self.n_pairs)

    def listed(self, i):
        return min(int(self.n_pairs[i]), self.rows.shape[1])

    def pairs_of(self, i):
        return [Pair(*(int(v) for v in row)) for row in self.rows[i, :self.listed(i)]]

    def region(self, i, k):
        """the points of M of pair k of row i"""
        return _points(self.regions[i, k], self.N)

    def find(self, i, anchor_b, anchor_w):
        """the Pair of row i with those anchors, or None"""
        for p in self.pairs_of(i):
            if (p.anchor_b, p.anchor_w) == (anchor_b, anchor_w):
                return p
        return None


def race_dev(size, records, idx, ask, region, rules, max_libs, max_region, max_nodes, max_pairs, lib):
    """sgo_race_dev on device tensors: (n_pairs int32 [n], rows int32 [n, max_pairs, 16], regions int32 [n, max_pairs, NW]) on the
    device; idx None: every record in order; ask / region None or device tensors int32 [n, 2] / [n, NW]"""
    import torch
    from . import _lib
    check_args(rules, max_libs, max_region, max_nodes, max_pairs)
    R = int(records.shape[0])
    n = R if idx is None else int(idx.shape[0])
    dev = records.device
    n_pairs = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = torch.zeros((n, int(max_pairs), 16), dtype=torch.int32, device=dev)
    regions = torch.zeros((n, int(max_pairs), lib.sgo_plane_words(size)), dtype=torch.int32, device=dev)
    _lib.check(lib.sgo_race_dev(C.c_int(size), C.c_int(n), _lib.ptr(records), C.c_int(R), _lib.ptr(idx), _lib.ptr(ask), _lib.ptr(region),
                                C.c_int(int(rules)), C.c_int(int(max_libs)), C.c_int(int(max_region)), C.c_int(int(max_nodes)),
                                C.c_int(int(max_pairs)), _lib.ptr(n_pairs), _lib.ptr(rows), _lib.ptr(regions), _lib.stream_ptr()), "sgo_race_dev")
    return n_pairs, rows, regions


def host_inputs(size, n, ask, region):
    """(ask int32 [n, 2] or None, region uint32 [n, NW] or None) as contiguous host arrays, checked"""
    NW = (size * size + 31) // 32
    if ask is not None:
        ask = np.ascontiguousarray(ask, np.int32).reshape(-1, 2)
        if len(ask) != n:
            raise ValueError("ask must hold two points (or -1, -1) per row")
    if region is not None:
        if ask is None:
            raise ValueError("a region goes with an asked pair")
        region = np.ascontiguousarray(region).view(np.uint32).reshape(-1, NW)
        if len(region) != n:
            raise ValueError("region must hold one bitset of NW words per row")
    return ask, region


def race(size, records, index=None, ask=None, region=None, rules=1, max_libs=4, max_region=8, max_nodes=1024, max_pairs=MAX_PAIRS):
    """sgo_race_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Race with one row per entry of
    `index` (None: every record in order); an index outside [0, R) gives n_pairs 0.  ask None: every pair in contact of every row;
    else two points per row ((-1, -1): enumerate that row), read in row i of `region` (uint32 [n, NW]) when given."""
    import torch
    from . import _lib
    check_args(rules, max_libs, max_region, max_nodes, max_pairs)
    records, _, idx, n = device_records(size, records, index)
    ask, region = host_inputs(size, n, ask, region)
    d_ask = None if ask is None else torch.from_numpy(ask).to(records.device)
    d_region = None if region is None else torch.from_numpy(region.view(np.int32)).to(records.device)
    n_pairs, rows, regions = race_dev(size, records, idx, d_ask, d_region, rules, max_libs, max_region, max_nodes, max_pairs, _lib.load())
    return Race(size, n_pairs.cpu().numpy(), rows.cpu().numpy(), regions.cpu().numpy().view(np.uint32))


def format_pair(p, vertex, N):
    """`sgo-race` line of a Pair: `D4 E4 libs 2 2 shared 0 empty 4 first to move wins black catch C1 save G1 white catch G1 save C1
    nodes 6 6 9 4`"""
    move = lambda a, skip: "none" if a < 0 else skip if a >= N else vertex(a)            # noqa: E731
    return "%s %s libs %d %d shared %d empty %d %s black catch %s save %s white catch %s save %s nodes %d %d %d %d" % (
        vertex(p.anchor_b), vertex(p.anchor_w), p.libs_b, p.libs_w, p.shared, p.region_empty, p.outcome, move(p.catch_b, "wait"),
        move(p.save_b, "pass"), move(p.catch_w, "wait"), move(p.save_w, "pass"), p.nodes_ab, p.nodes_db, p.nodes_aw, p.nodes_dw)


# ---- game review: was the played move the move that decides an unsettled race? -------------------------------------------------
def winning_moves(pairs, colour, N):
    """{point: anchor of the racer it decides} of the side `colour` (+1 black, -1 white) from the Pair list of a position: its
    saving move of every own racer that is unsettled and its catching move of every opposing racer that is unsettled; passes and
    waits are left out.  Where two racers name one point the first listed stays."""
    out = {}
    for p in pairs:
        own = (p.black, p.anchor_b, p.save_b) if colour > 0 else (p.white, p.anchor_w, p.save_w)
        other = (p.white, p.anchor_w, p.catch_w) if colour > 0 else (p.black, p.anchor_b, p.catch_b)
        for word, anchor, move in (own, other):
            if word == "unsettled" and 0 <= move < N:
                out.setdefault(move, anchor)
    return out


def review_flags(size, action, colour, before, vertex=str):
    """Flags of one move by `colour` from the Pair list of the position in front of it:
      `wins-race V`         the move is the catching or saving move of a pair whose racer V of the mover's interest is unsettled;
      `missed-race V at K`  such a move K existed and another was played (one flag per racer; none when the move won a race).
    These are flags from a bounded reader, not verdicts: unknown and open rows are never flagged."""
    N = size * size
    moves = winning_moves(before, colour, N)
    if action in moves:
        return ["wins-race %s" % vertex(moves[action])]
    flags, seen = [], set()
    for k in sorted(moves):
        if moves[k] not in seen:
            seen.add(moves[k])
            flags.append("missed-race %s at %s" % (vertex(moves[k]), vertex(k)))
    return flags


# ---- record statistics: pairs per position, verdict shares, how often the recorded move decided a race --------------------------
def bucket_table(ply, actions, colours, rows, n_pairs, N, width=20):
    """The table of `records --race` from one entry per position: ply int [n] (0-based move number), actions int [n], colours int [n]
    (+1 / -1, the mover), rows int32 [n, P, 16], n_pairs int [n].  A list of dicts per bucket of `width` plies in ascending order:
    {"from", "to", "plies", "pairs" (listed rows), "racers" (two per read pair), "safe", "unsettled", "caught", "unknown" (racers of
    each verdict), "chances" (positions with a catching or saving move for the mover), "took" (of those, the recorded move is one)}."""
    ply, actions, colours = np.asarray(ply, np.int64), np.asarray(actions, np.int64), np.asarray(colours, np.int64)
    rows, n_pairs = np.asarray(rows, np.int64), np.asarray(n_pairs, np.int64)
    listed = np.arange(rows.shape[1])[None, :] < np.minimum(n_pairs, rows.shape[1])[:, None]
    st = rows[:, :, 6]
    read = listed & ((st & (OPEN | NO_PAIR)) == 0)
    words = {}
    for name, bits in (("b", st & 255), ("w", (st >> WHITE_SHIFT) & 255)):
        unk = (bits & (A_UNKNOWN | D_UNKNOWN)) != 0
        words[name] = {"unknown": read & unk, "safe": read & ~unk & ((bits & A_CAUGHT) == 0),
                       "unsettled": read & ~unk & ((bits & A_CAUGHT) != 0) & ((bits & D_CAUGHT) == 0),
                       "caught": read & ~unk & ((bits & A_CAUGHT) != 0) & ((bits & D_CAUGHT) != 0)}
    black = (colours > 0)[:, None]
    # the mover's moves of interest: save its own unsettled racer, catch the other's
    own_uns = np.where(black, words["b"]["unsettled"], words["w"]["unsettled"])
    oth_uns = np.where(black, words["w"]["unsettled"], words["b"]["unsettled"])
    save = np.where(black, rows[:, :, 9], rows[:, :, 11])
    catch = np.where(black, rows[:, :, 10], rows[:, :, 8])
    ok_s, ok_c = own_uns & (save >= 0) & (save < N), oth_uns & (catch >= 0) & (catch < N)
    chance = (ok_s | ok_c).any(axis=1)
    took = ((ok_s & (save == actions[:, None])) | (ok_c & (catch == actions[:, None]))).any(axis=1)
    out = []
    for b in sorted(set((ply // width).tolist())):
        sel = (ply // width) == b
        r = {"from": int(b * width + 1), "to": int((b + 1) * width), "plies": int(sel.sum()), "pairs": int(listed[sel].sum()),
             "racers": 2 * int(read[sel].sum()), "chances": int(chance[sel].sum()), "took": int(took[sel].sum())}
        for v in VERDICTS:
            r[v] = int(words["b"][v][sel].sum() + words["w"][v][sel].sum())
        out.append(r)
    return out


def format_bucket_table(table):
    lines = ["moves      plies  pairs/ply   safe  unsettled  caught  unknown  chances  took"]
    for r in table:
        n = max(1, r["racers"])
        lines.append("%4d-%-4d  %5d  %9.2f  %4.0f%%  %8.0f%%  %5.0f%%  %6.0f%%  %7d  %4d" % (
            r["from"], r["to"], r["plies"], r["pairs"] / max(1, r["plies"]), 100.0 * r["safe"] / n, 100.0 * r["unsettled"] / n,
            100.0 * r["caught"] / n, 100.0 * r["unknown"] / n, r["chances"], r["took"]))
    return "\n".join(lines)
