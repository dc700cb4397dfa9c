"""Move outcomes on the device (include/sgo.h "move outcomes", csrc/sgo_moves.hip): per position and per point of the board what
one ply by the side to move (or, side=1, by the other colour) on that point would do -- what it captures, how large the new chain
is and how many liberties it keeps, which chains it joins, which opponent chains it puts in atari -- and a per-position summary.
One ply, no reading: ladders stay with tactics.py.

    from sejonggo_amd.moves import moves
    v = moves(19, records)                   # packed records uint32 [R, 16 * NW], host or device
    m = v.move(0, 72); m.allowed, m.captures, m.libs, m.self_atari, m.gives_atari, m.escapes
    v.counts[0]                              # allowed, capturing, max_captured, max_capture_move, self_atari, atari_giving, ...

records.RecordSet.moves() reads the played move of every position of a game collection, engine.SessionEngine.moves(slots) the
positions of session slots; GTP's `sgo-moves`, `python -m sejonggo_amd.review --moves` and `python -m sejonggo_amd.records --moves`
stand on them."""
import collections
import ctypes as C

import numpy as np

from ._packed import device_records

ALLOWED, OCCUPIED, KO, SUICIDE = 1, 2, 4, 8
COUNTS = ("allowed", "capturing", "max_captured", "max_capture_move", "self_atari", "atari_giving", "escapes", "forbidden_sound")
KINDS = ("capture", "atari", "escape", "selfatari", "forbidden", "all")


class Move(collections.namedtuple("Move", "flags captured size libs joined weakest ataris atari_stones")):
    """One row of the table.  The properties are the predicates of the per-record counts; the first five of them (`captures`,
    `self_atari`, `gives_atari`, `escapes`, and `allowed` itself) hold for ALLOWED points only, as the counts do."""
    __slots__ = ()

    @property
    def allowed(self):
        return bool(self.flags & ALLOWED)

    @property
    def occupied(self):
        return bool(self.flags & OCCUPIED)

    @property
    def ko(self):
        return bool(self.flags & KO)

    @property
    def suicide(self):
        return bool(self.flags & SUICIDE)

    @property
    def captures(self):
        return self.allowed and self.captured > 0

    @property
    def self_atari(self):
        return self.allowed and self.libs == 1 and self.captured == 0

    @property
    def gives_atari(self):
        return self.allowed and self.ataris > 0

    @property
    def escapes(self):
        return self.allowed and self.weakest == 1 and self.libs >= 2

    @property
    def forbidden_sound(self):
        """an empty point the inherited rule forbids although the stone would stand"""
        return not self.flags & (ALLOWED | OCCUPIED | KO | SUICIDE)

    def is_kind(self, kind):
        return {"capture": self.captures, "atari": self.gives_atari, "escape": self.escapes, "selfatari": self.self_atari,
                "forbidden": self.forbidden_sound, "all": not self.occupied}[kind]


class Moves(object):
    """rows int16 [n, N, 8] ({flags, captured, size, libs, joined, weakest, ataris, atari_stones} per point), counts int32 [n, 8]
    (COUNTS)."""

    def __init__(self, size, rows, counts, status=None):
        self.S, self.N = size, size * size
        self.rows, self.counts = np.asarray(rows, dtype=np.int16), np.asarray(counts, dtype=np.int32)
        self.status = status

    def __len__(self):
        return len(self.counts)

    def move(self, i, a):
        return Move(*(int(v) for v in self.rows[i, a]))

    def count(self, i, name):
        return int(self.counts[i, COUNTS.index(name)])

    def points(self, i, kind="all"):
        """[(a, Move)] of the points of row i of one of KINDS, ascending"""
        out = []
        for a in range(self.N):
            m = self.move(i, a)
            if m.is_kind(kind):
                out.append((a, m))
        return out


def moves_dev(size, records, idx, side, lib):
    """sgo_moves_dev on device tensors: (rows int16 [n, N, 8], counts int32 [n, 8]) on the device; idx None: every record in order"""
    import torch
    from . import _lib
    R = int(records.shape[0])
    n = R if idx is None else int(idx.shape[0])
    # the kernel writes every word of every row (the zero row for an index out of range): nothing to clear first
    rows = torch.empty((n, size * size, 8), dtype=torch.int16, device=records.device)
    counts = torch.empty((n, 8), dtype=torch.int32, device=records.device)
    _lib.check(lib.sgo_moves_dev(C.c_int(size), C.c_int(n), _lib.ptr(records), C.c_int(R), _lib.ptr(idx), C.c_int(int(side)), _lib.ptr(rows),
                                 _lib.ptr(counts), _lib.stream_ptr()), "sgo_moves_dev")
    return rows, counts


def moves(size, records, index=None, side=0):
    """sgo_moves_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Moves with one row per entry
    of `index` (None: every record in order); an index outside [0, R) gives the zero row.  side 0: the side to move, 1: the other."""
    from . import _lib
    records, _, idx, _ = device_records(size, records, index)
    rows, counts = moves_dev(size, records, idx, side, _lib.load())
    return Moves(size, rows.cpu().numpy(), counts.cpu().numpy())


def format_move(m, vertex):
    """`sgo-moves` line of a Move at the point named `vertex`: `D4 captures 3 size 1 liberties 2 joins 0 ataris 1`, with the words
    `ko`, `suicide`, `forbidden` appended where they hold"""
    text = "%s captures %d size %d liberties %d joins %d ataris %d" % (vertex, m.captured, m.size, m.libs, m.joined, m.ataris)
    for word, on in (("ko", m.ko), ("suicide", m.suicide), ("forbidden", m.forbidden_sound)):
        if on:
            text += " " + word
    return text


def format_kind(v, i, kind, vertex):
    """`sgo-moves` text of row i of a Moves: one format_move line per point of the kind, ascending; vertex(a) names a point"""
    return "\n".join(format_move(m, vertex(a)) for a, m in v.points(i, kind))


# ---- game review: what the played move did, from its row in the position before it ------------------------------------------------
def review_flags(size, action, row, counts, vertex=str):
    """Flags of one played move from its table row (int16 [8]) and the counts (int32 [8]) of the position before it, side 0:
    `captures N`           captured >= 1;
    `atari`                ataris > 0;
    `escape`               weakest == 1 and libs >= 2;
    `self-atari`           libs == 1, captured == 0 and size >= 2 (a one-stone throw-in is not flagged);
    `missed-capture K at V` the move captured nothing while max_captured = K >= 3, V = vertex(max_capture_move).
    A pass gets no flag.  These are flags, not verdicts: one ply is looked at, nothing is read out."""
    if not 0 <= action < size * size:
        return []
    m = Move(*(int(v) for v in row))
    flags = []
    if m.captured >= 1:
        flags.append("captures %d" % m.captured)
    if m.ataris > 0:
        flags.append("atari")
    if m.weakest == 1 and m.libs >= 2:
        flags.append("escape")
    if m.libs == 1 and m.captured == 0 and m.size >= 2:
        flags.append("self-atari")
    if m.captured == 0 and int(counts[2]) >= 3:
        flags.append("missed-capture %d at %s" % (int(counts[2]), vertex(int(counts[3]))))
    return flags


# ---- record statistics: what the played moves did, per 20-move bucket, beside what the allowed moves of the same positions do -----
PLAYED = ("capture", "atari", "escape", "self_atari")


def bucket_table(ply, actions, played, counts, size, width=20):
    """The table of `records --moves` from one entry per position: ply int [n] (0-based move number), actions int [n], played int16
    [n, 8] (the row of the played move; ignored for a pass), counts int32 [n, 8].  A list of dicts per bucket of `width` plies in
    ascending order: {"from", "to", "plies", "passes", "played": {kind: share of the non-pass plies}, "allowed": {kind: mean over
    those positions of count / allowed (positions without an allowed point left out)}, "forbidden_sound", "positions_forbidden"}.
    Played moves are counted by the predicates of the counts: capture = captured > 0, atari = ataris > 0, escape = weakest == 1 and
    libs >= 2, self_atari = libs == 1 and captured == 0."""
    ply, actions = np.asarray(ply, np.int64), np.asarray(actions, np.int64)
    played, counts = np.asarray(played, np.int64).reshape(-1, 8), np.asarray(counts, np.int64).reshape(-1, 8)
    N = size * size
    real = (actions >= 0) & (actions < N)
    hit = {"capture": played[:, 1] > 0, "atari": played[:, 6] > 0, "escape": (played[:, 5] == 1) & (played[:, 3] >= 2),
           "self_atari": (played[:, 3] == 1) & (played[:, 1] == 0)}
    col = {"capture": 1, "atari": 5, "escape": 6, "self_atari": 4}
    out = []
    for b in sorted(set((ply // width).tolist())):
        sel = (ply // width) == b
        mv = sel & real
        k = int(mv.sum())
        pos = mv & (counts[:, 0] > 0)
        row = {"from": int(b * width + 1), "to": int((b + 1) * width), "plies": int(sel.sum()), "passes": int(sel.sum()) - k,
               "played": {}, "allowed": {}, "forbidden_sound": int(counts[sel, 7].sum()), "positions_forbidden": int((counts[sel, 7] > 0).sum())}
        for kind in PLAYED:
            row["played"][kind] = float(hit[kind][mv].sum()) / k if k else 0.0
            row["allowed"][kind] = float((counts[pos, col[kind]] / counts[pos, 0]).mean()) if pos.any() else 0.0
        out.append(row)
    return out


def format_bucket_table(table):
    lines = ["moves      plies  capture  (allowed)  atari  (allowed)  escape  (allowed)  self-atari  (allowed)  forbidden-sound  positions"]
    for r in table:
        cells = "".join("  %6.3f   (%6.3f)" % (r["played"][k], r["allowed"][k]) for k in PLAYED)
        lines.append("%4d-%-4d  %6d%s  %8d  %8d" % (r["from"], r["to"], r["plies"], cells, r["forbidden_sound"], r["positions_forbidden"]))
    return "\n".join(lines)
