"""Life and death on the device (include/sgo.h "life and death", csrc/sgo_solve.hip): per position the enclosed chains (or the one
chain asked for), the region M each is read in, and for each whether an exhaustive reader bounded by M kills it -- with the attacker
moving first (`kill_move`) and even with the defender moving first -- with pass-alive as the terminal for "lives".  A bounded
reader, not a proof about the game: no transposition table, the one-ply ko approximation, a chain judged alone, and "alive" means
"the attacker cannot capture it inside M" for the chosen rule set.

    from sejonggo_amd.solve import solve
    v = solve(19, records)                       # packed records uint32 [R, 16 * NW], host or device; every enclosed chain
    for t in v.targets_of(0): print(t.anchor, t.verdict, t.kill_move, t.live_move, t.nodes_a, t.nodes_d)
    v = solve(19, records, ask=[72])             # the chain on point 72 of record 0, in its default region
    v.region(0, 0)                               # the points of M

records.RecordSet.solve() reads every position of a game collection, engine.SessionEngine.solve(slots) the positions of session
slots; GTP's `sgo-solve`, `python -m sejonggo_amd.review --solve` and `python -m sejonggo_amd.records --solve` stand on them."""
import collections
import ctypes as C

import numpy as np

from ._packed import device_records, points as _points

A_DEAD, D_DEAD, A_UNKNOWN, D_UNKNOWN, D_RAN, OPEN, NO_STONE = 1, 2, 4, 8, 16, 32, 64
MAX_REGION, MAX_NODES, MAX_TARGETS = 32, 65536, 64
VERDICTS = ("alive", "unsettled", "dead", "unknown", "open")


def verdict_of(status):
    """`alive` (A not DEAD), `unsettled` (A DEAD, D not DEAD), `dead` (both DEAD), `unknown` (a query ran out of its budget),
    `open` (no query ran: the region has no empty point or more than max_region); None for an asked point without a stone"""
    status = int(status)
    if status & NO_STONE:
        return None
    if status & OPEN:
        return "open"
    if status & (A_UNKNOWN | D_UNKNOWN):
        return "unknown"
    if not status & A_DEAD:
        return "alive"
    return "dead" if status & D_DEAD else "unsettled"


class Target(collections.namedtuple("Target", "anchor colour region_empty status kill_move live_move nodes_a nodes_d")):
    """One row of the target table.  colour +1 black / -1 white; kill_move / live_move -1: none; live_move N: the pass; kill_move N: the
    attacker's wait (it only waits out a ko ban at the root)."""
    __slots__ = ()

    @property
    def verdict(self):
        return verdict_of(self.status)


def check_args(rules, max_region, max_nodes, max_targets):
    if rules not in (0, 1):
        raise ValueError("rules must be 0 (inherited) or 1 (sound)")
    if not 1 <= int(max_region) <= MAX_REGION:
        raise ValueError("max_region must be in [1, %d]" % MAX_REGION)
    if not 1 <= int(max_nodes) <= MAX_NODES:
        raise ValueError("max_nodes must be in [1, %d]" % MAX_NODES)
    if not 1 <= int(max_targets) <= MAX_TARGETS:
        raise ValueError("max_targets must be in [1, %d]" % MAX_TARGETS)


class Solve(object):
    """n_targets int32 [n] (the true number), rows int32 [n, max_targets, 8], regions uint32 [n, max_targets, NW] (the first
    min(n_targets, max_targets) of each position)."""

    def __init__(self, size, n_targets, rows, regions, status=None):
        self.S, self.N = size, size * size
        self.n_targets, self.rows = np.asarray(n_targets, dtype=np.int32), np.asarray(rows, dtype=np.int32)
        self.regions = np.asarray(regions, dtype=np.uint32)
        self.status = status

    def __len__(self):
        return len(self.n_targets)

    def listed(self, i):
        return min(int(self.n_targets[i]), self.rows.shape[1])

    def targets_of(self, i):
        return [Target(*(int(v) for v in row)) for row in self.rows[i, :self.listed(i)]]

    def region(self, i, k):
        """the points of M of target k of row i"""
        return _points(self.regions[i, k], self.N)

    def find(self, i, anchor):
        """the Target of row i with that anchor, or None"""
        for t in self.targets_of(i):
            if t.anchor == anchor:
                return t
        return None


def solve_dev(size, records, idx, ask, region, rules, max_region, max_nodes, max_targets, lib):
    """sgo_solve_dev on device tensors: (n_targets int32 [n], rows int32 [n, max_targets, 8], regions int32 [n, max_targets, NW])
    on the device; idx None: every record in order; ask / region None or device tensors int32 [n] / [n, NW]"""
    import torch
    from . import _lib
    check_args(rules, max_region, max_nodes, max_targets)
    R = int(records.shape[0])
    n = R if idx is None else int(idx.shape[0])
    dev = records.device
    n_targets = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = torch.zeros((n, int(max_targets), 8), dtype=torch.int32, device=dev)
    regions = torch.zeros((n, int(max_targets), lib.sgo_plane_words(size)), dtype=torch.int32, device=dev)
    _lib.check(lib.sgo_solve_dev(C.c_int(size), C.c_int(n), _lib.ptr(records), C.c_int(R), _lib.ptr(idx), _lib.ptr(ask), _lib.ptr(region),
                                 C.c_int(int(rules)), C.c_int(int(max_region)), C.c_int(int(max_nodes)), C.c_int(int(max_targets)),
                                 _lib.ptr(n_targets), _lib.ptr(rows), _lib.ptr(regions), _lib.stream_ptr()), "sgo_solve_dev")
    return n_targets, rows, regions


def host_inputs(size, n, ask, region):
    """(ask int32 [n] or None, region uint32 [n, NW] or None) as contiguous host arrays, checked"""
    NW = (size * size + 31) // 32
    if ask is not None:
        ask = np.ascontiguousarray(ask, np.int32).reshape(-1)
        if len(ask) != n:
            raise ValueError("ask must hold one point (or -1) per row")
    if region is not None:
        if ask is None:
            raise ValueError("a region goes with an asked point")
        region = np.ascontiguousarray(region).view(np.uint32).reshape(-1, NW)
        if len(region) != n:
            raise ValueError("region must hold one bitset of NW words per row")
    return ask, region


def region_words(size, pts):
    """uint32 [NW]: the bitset of a list of points"""
    w = np.zeros((size * size + 31) // 32, np.uint32)
    for a in pts:
        w[a >> 5] |= np.uint32(1 << (a & 31))
    return w


def solve(size, records, index=None, ask=None, region=None, rules=1, max_region=12, max_nodes=4096, max_targets=MAX_TARGETS):
    """sgo_solve_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Solve with one row per entry
    of `index` (None: every record in order); an index outside [0, R) gives n_targets 0.  ask None: every enclosed chain of every
    row; else one point per row (-1: enumerate that row), read in row i of `region` (uint32 [n, NW]) when given."""
    import torch
    from . import _lib
    check_args(rules, max_region, max_nodes, max_targets)
    records, _, idx, n = device_records(size, records, index)
    ask, region = host_inputs(size, n, ask, region)
    d_ask = None if ask is None else torch.from_numpy(ask).to(records.device)
    d_region = None if region is None else torch.from_numpy(region.view(np.int32)).to(records.device)
    n_targets, rows, regions = solve_dev(size, records, idx, d_ask, d_region, rules, max_region, max_nodes, max_targets, _lib.load())
    return Solve(size, n_targets.cpu().numpy(), rows.cpu().numpy(), regions.cpu().numpy().view(np.uint32))


def format_target(t, vertex, N):
    """`sgo-solve` line of a Target: `D4 black empty 5 unsettled kill E1 live E1 nodes 22 17`"""
    move = lambda a, skip: "none" if a < 0 else skip if a >= N else vertex(a)            # noqa: E731
    return "%s %s empty %d %s kill %s live %s nodes %d %d" % (
        vertex(t.anchor), "black" if t.colour > 0 else "white", t.region_empty, t.verdict, move(t.kill_move, "wait"), move(t.live_move, "pass"),
        t.nodes_a, t.nodes_d)


def format_board(size, stones, region_points, t):
    """S lines from the top row down, one cell per point: X / O a black / white stone, * an empty point of M, K the kill move, L the
    live move (! where they are the same point), . anything else; stones int8 [N] (+1 / -1)"""
    M = set(region_points)
    cell = []
    for a in range(size * size):
        if stones[a]:
            cell.append("X" if stones[a] > 0 else "O")
        elif a == t.kill_move and a == t.live_move:
            cell.append("!")
        elif a == t.kill_move:
            cell.append("K")
        elif a == t.live_move:
            cell.append("L")
        else:
            cell.append("*" if a in M else ".")
    return "\n".join(" ".join(cell[y * size:(y + 1) * size]) for y in range(size))


# ---- game review: what the played move did to the chains the reader decides, from the tables before and after it -----------------
def review_flags(size, action, colour, stones_before, before, stones_after, after, vertex=str):
    """Flags of one move by `colour` from the stones (int8 [N]) and the Target lists of the position before and after it.  A chain
    is followed by its stones: the `after` target of a `before` target is the one whose anchor lies on a point the chain held.
      `kills V`           an opponent chain V that was unsettled or alive before is dead after (or gone from the board);
      `saves V`           an own chain V that was unsettled before is alive after;
      `missed-kill V at K`  an opponent chain V was unsettled before with kill_move K, the move was not K, and it is not dead after;
      `missed-save V at K`  an own chain V was unsettled before with live_move K, the move was not K, and it is not alive after.
    These are flags from a bounded reader, not verdicts: unknown and open rows are never flagged."""
    from .tactics import chain_points
    N, flags = size * size, []
    for t in before:
        if t.verdict not in ("unsettled", "alive"):
            continue
        pts = chain_points(size, stones_before, t.anchor)
        now = None
        for u in after:
            if u.anchor in pts and u.colour == t.colour:
                now = u
        gone = stones_after[t.anchor] != t.colour
        name = vertex(t.anchor)
        if t.colour == -colour:
            killed = gone or (now is not None and now.verdict == "dead")
            if killed:
                flags.append("kills %s" % name)
            elif t.verdict == "unsettled" and action != t.kill_move and 0 <= t.kill_move < N:
                flags.append("missed-kill %s at %s" % (name, vertex(t.kill_move)))
        elif t.verdict == "unsettled":
            saved = not gone and (now is None or now.verdict == "alive")
            if saved:
                flags.append("saves %s" % name)
            elif action != t.live_move and 0 <= t.live_move < N:
                flags.append("missed-save %s at %s" % (name, vertex(t.live_move)))
    return flags


# ---- record statistics: how often the recorded move was the kill or the live move, per 20-move bucket --------------------------
def bucket_table(ply, actions, rows, n_targets, width=20):
    """The table of `records --solve` from one entry per position: ply int [n] (0-based move number), actions int [n], rows int32
    [n, T, 8], n_targets int [n].  A list of dicts per bucket of `width` plies in ascending order: {"from", "to", "plies", "rows"
    (listed table rows), "unsettled" (positions that hold an unsettled chain), "took" (of those, the recorded move is the kill_move
    or live_move of one), "unknown" (rows that ended unknown)}."""
    ply, actions = np.asarray(ply, np.int64), np.asarray(actions, np.int64)
    rows, n_targets = np.asarray(rows, np.int64), np.asarray(n_targets, np.int64)
    listed = np.arange(rows.shape[1])[None, :] < np.minimum(n_targets, rows.shape[1])[:, None]
    st = rows[:, :, 3]
    unknown = listed & ((st & (A_UNKNOWN | D_UNKNOWN)) != 0)
    uns = listed & ~unknown & ((st & A_DEAD) != 0) & ((st & D_DEAD) == 0) & ((st & (OPEN | NO_STONE)) == 0)
    hit = uns & ((rows[:, :, 4] == actions[:, None]) | (rows[:, :, 5] == actions[:, None]))
    out = []
    for b in sorted(set((ply // width).tolist())):
        sel = (ply // width) == b
        out.append({"from": int(b * width + 1), "to": int((b + 1) * width), "plies": int(sel.sum()), "rows": int(listed[sel].sum()),
                    "unsettled": int(uns[sel].any(axis=1).sum()), "took": int(hit[sel].any(axis=1).sum()),
                    "unknown": int(unknown[sel].sum())})
    return out


def format_bucket_table(table):
    lines = ["moves      plies   rows  unsettled  took  unknown-share"]
    for r in table:
        lines.append("%4d-%-4d  %5d  %5d  %9d  %4d  %12.1f%%" % (r["from"], r["to"], r["plies"], r["rows"], r["unsettled"], r["took"],
                                                                100.0 * r["unknown"] / max(1, r["rows"])))
    return "\n".join(lines)
