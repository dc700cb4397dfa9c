"""Securing moves on the device (include/sgo.h "securing moves", csrc/sgo_secure.hip): per position and per empty point what ONE
more stone of the side to move (or, side=1, of the other colour) makes pass-alive -- the ply of the rules, then unconditional life
on the position after it -- and per position the best such stone with the life sets before and after it.  A proof about one ply:
"after this stone, these stones can never be captured".  What the opponent's answer undoes is not read.

    from sejonggo_amd.secure import secure
    v = secure(19, records)                  # packed records uint32 [R, 16 * NW], host or device
    v.best(0), v.gain(0, 72), v.securing(0, 2), v.harmful(0), v.secured(0)
    v.counts[0]                              # base_alive, base_terr, base_dead, allowed, securing, best_gain, best_move, harmful

records.RecordSet.secure() reads every position of a game collection, engine.SessionEngine.secure(slots) the positions of session
slots; GTP's `sgo-secure`, `python -m sejonggo_amd.review --secure` and `python -m sejonggo_amd.records --secure` stand on them."""
import ctypes as C

import numpy as np

from ._packed import device_records, points as _points
from .moves import ALLOWED, OCCUPIED

COUNTS = ("base_alive", "base_terr", "base_dead", "allowed", "securing", "best_gain", "best_move", "harmful")
MIN_GAIN = 2        # a stone that merely extends a living chain gains 1: noise for a reader


class Secure(object):
    """table int16 [n, N, 4] ({flags, alive, terr, dead} per point), sets uint32 [n, 4, NW] (alive, terr of the position; alive,
    terr after best_move), counts int32 [n, 8] (COUNTS)."""

    def __init__(self, size, table, sets, counts, status=None):
        self.S, self.N = size, size * size
        self.table, self.sets = np.asarray(table, dtype=np.int16), np.asarray(sets, dtype=np.uint32)
        self.counts = np.asarray(counts, dtype=np.int32)
        self.status = status

    def __len__(self):
        return len(self.counts)

    def count(self, i, name):
        return int(self.counts[i, COUNTS.index(name)])

    def base(self, i):
        return int(self.counts[i, 0]) + int(self.counts[i, 1])

    def gain(self, i, a):
        """alive + terr after a stone on the empty point a, less the same of the position; None on an occupied point"""
        f, alive, terr, _ = (int(v) for v in self.table[i, a])
        return None if f & OCCUPIED else alive + terr - self.base(i)

    def gains(self, i):
        """(gain int64 [N], allowed bool [N]) of row i; the gain stands as 0 where the point is not ALLOWED"""
        t = self.table[i].astype(np.int64)
        ok = (t[:, 0] & ALLOWED) != 0
        return np.where(ok, t[:, 1] + t[:, 2] - self.base(i), 0), ok

    def best(self, i):
        """(best_move, best_gain), or None when nothing is ALLOWED"""
        return (self.count(i, "best_move"), self.count(i, "best_gain")) if self.count(i, "allowed") else None

    def securing(self, i, min_gain=1):
        """[(a, gain)] of the ALLOWED points with gain >= min_gain, ascending in a"""
        g, ok = self.gains(i)
        return [(int(a), int(g[a])) for a in np.flatnonzero(ok & (g >= min_gain))]

    def harmful(self, i):
        """[(a, gain)] of the ALLOWED points with gain < 0, ascending in a"""
        g, ok = self.gains(i)
        return [(int(a), int(g[a])) for a in np.flatnonzero(ok & (g < 0))]

    def safe(self, i, after=False):
        """the points of alive | terr of the position, or of the position after best_move"""
        k = 2 if after else 0
        return _points(self.sets[i, k] | self.sets[i, k + 1], self.N)

    def secured(self, i):
        """the stones and points that are safe after best_move and were not before"""
        return sorted(set(self.safe(i, True)) - set(self.safe(i)))


def secure_dev(size, records, idx, side, lib):
    """sgo_secure_dev on device tensors: (table int16 [n, N, 4], sets int32 [n, 4, NW], counts int32 [n, 8]) on the device; idx None:
    every record in order"""
    import torch
    from . import _lib
    R = int(records.shape[0])
    n = R if idx is None else int(idx.shape[0])
    # the kernels write every word of every row (the zero row for an index out of range): nothing to clear first
    table = torch.empty((n, size * size, 4), dtype=torch.int16, device=records.device)
    sets = torch.empty((n, 4, lib.sgo_plane_words(size)), dtype=torch.int32, device=records.device)
    counts = torch.empty((n, 8), dtype=torch.int32, device=records.device)
    _lib.check(lib.sgo_secure_dev(C.c_int(size), C.c_int(n), _lib.ptr(records), C.c_int(R), _lib.ptr(idx), C.c_int(int(side)), _lib.ptr(table),
                                  _lib.ptr(sets), _lib.ptr(counts), _lib.stream_ptr()), "sgo_secure_dev")
    return table, sets, counts


def secure(size, records, index=None, side=0):
    """sgo_secure_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Secure with one row per
    entry of `index` (None: every record in order); an index outside [0, R) gives the zero row.  side 0: the side to move, 1: the
    other colour."""
    from . import _lib
    records, _, idx, _ = device_records(size, records, index)
    table, sets, counts = secure_dev(size, records, idx, side, _lib.load())
    return Secure(size, table.cpu().numpy(), sets.cpu().numpy().view(np.uint32), counts.cpu().numpy())


def format_board(v, i, stones, vertex, min_gain=MIN_GAIN):
    """`sgo-secure` text of row i of a Secure: S lines from the top row down with one cell per point -- X / O a black / white stone
    (stones int8 [N], +1 / -1), the gain on an ALLOWED point whose gain is >= min_gain, - on a harmful one, . anything else -- then
    `base B allowed A securing K harmful H`, and `best V gain G secures ...` with the points that become safe (or `best none`)."""
    S, N = v.S, v.N
    g, ok = v.gains(i)
    cell = []
    for a in range(N):
        if stones[a]:
            cell.append("X" if stones[a] > 0 else "O")
        elif ok[a] and g[a] < 0:
            cell.append("-")
        elif ok[a] and g[a] >= min_gain:
            cell.append(str(int(g[a])))
        else:
            cell.append(".")
    lines = ["".join("%4s" % c for c in cell[y * S:(y + 1) * S]) for y in range(S)]
    lines.append("base %d allowed %d securing %d harmful %d" % (v.base(i), v.count(i, "allowed"), len(v.securing(i, min_gain)), v.count(i, "harmful")))
    best = v.best(i)
    if best is None or best[1] < min_gain:
        lines.append("best none")
    else:
        lines.append("best %s gain %d secures %s" % (vertex(best[0]), best[1], " ".join(vertex(a) for a in v.secured(i))))
    return "\n".join(lines)


# ---- game review: what the played move proved, from its row in the position before it ----------------------------------------------
def review_flags(size, action, row, counts, vertex=str, min_gain=MIN_GAIN):
    """Flags of one played move from its table row (int16 [4]) and the counts (int32 [8]) of the position before it, side 0:
    `secures K`            the move's gain K is >= min_gain;
    `missed-secure K at V` best_gain = K >= min_gain and the move gains less than half of it, V = vertex(best_move);
    `destroys K`           the move's gain is -K < 0.
    A pass and a move on an occupied point count with gain 0.  These are flags from a proof about one ply, not a verdict on the
    move: what the opponent's answer undoes is not read."""
    played = 0 <= action < size * size and not int(row[0]) & OCCUPIED
    gain = int(row[1]) + int(row[2]) - int(counts[0]) - int(counts[1]) if played else 0
    flags = []
    if gain >= min_gain:
        flags.append("secures %d" % gain)
    best = int(counts[5]) if int(counts[3]) else 0
    if best >= min_gain and 2 * gain < best:
        flags.append("missed-secure %d at %s" % (best, vertex(int(counts[6]))))
    if gain < 0:
        flags.append("destroys %d" % -gain)
    return flags


# ---- record statistics: how often the recorded move took what the board offered, per 20-move bucket -------------------------------
def bucket_table(ply, actions, played, counts, size, width=20, min_gain=MIN_GAIN):
    """The table of `records --secure` from one entry per position: ply int [n] (0-based move number), actions int [n], played
    int16 [n, 4] (the row of the played move; ignored for a pass), counts int32 [n, 8].  A list of dicts per bucket of `width` plies
    in ascending order: {"from", "to", "plies", "proved" (positions with base > 0), "offered" (positions whose best_gain is >=
    min_gain), "took_best" (of those, the played move's gain equals best_gain), "took_any" (its gain is >= min_gain),
    "harmful_played" (played moves with gain < 0)}."""
    ply, actions = np.asarray(ply, np.int64), np.asarray(actions, np.int64)
    played, counts = np.asarray(played, np.int64).reshape(-1, 4), np.asarray(counts, np.int64).reshape(-1, 8)
    real = (actions >= 0) & (actions < size * size) & ((played[:, 0] & OCCUPIED) == 0)
    base = counts[:, 0] + counts[:, 1]
    gain = np.where(real, played[:, 1] + played[:, 2] - base, 0)
    offered = (counts[:, 3] > 0) & (counts[:, 5] >= min_gain)
    out = []
    for b in sorted(set((ply // width).tolist())):
        sel = (ply // width) == b
        out.append({"from": int(b * width + 1), "to": int((b + 1) * width), "plies": int(sel.sum()), "proved": int((sel & (base > 0)).sum()),
                    "offered": int((sel & offered).sum()), "took_best": int((sel & offered & real & (gain == counts[:, 5])).sum()),
                    "took_any": int((sel & offered & real & (gain >= min_gain)).sum()),
                    "harmful_played": int((sel & real & (gain < 0)).sum())})
    return out


def format_bucket_table(table):
    lines = ["moves      plies  proved  offered  took-best  took-any  harmful-played"]
    for r in table:
        lines.append("%4d-%-4d  %5d  %6d  %7d  %9d  %8d  %14d" % (r["from"], r["to"], r["plies"], r["proved"], r["offered"], r["took_best"],
                                                                  r["took_any"], r["harmful_played"]))
    return "\n".join(lines)
