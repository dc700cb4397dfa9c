"""Superko on the device (include/sgo.h "superko", csrc/sgo_superko.hip): per position of a game and per empty point whether one
ply of the side to move there recreates a position the game has already held (positional: the same stones; situational: the same
stones and the same side to move), and how many plies back.  The one analysis that reads a record AND the records of its game before
it: row i names a record and the FIRST record of its game.

    from sejonggo_amd.superko import superko
    v = superko(19, records, index, first, rule=0)     # packed records uint32 [R, 16 * NW], host or device
    v.repeat(0), v.extra(0), v.back[0, 72], v.count(0, "seen")
    v.counts[0]                                        # repeat, extra, max_back, max_back_point, seen, history, refuted, truncated

`extra` holds the points superko forbids and the inherited one-ply ko rule allows; `legal_superko` is a drop-in legal set.
records.RecordSet.superko() reads every position of a game collection; GTP's `sgo-superko` and `--superko`, `python -m
sejonggo_amd.review --superko` and `python -m sejonggo_amd.records --superko` stand on it.  There is no session form: a session slot
holds seven positions of history, not the game; gtp.DeviceSejongGoEngine.superko replays its move list."""
import ctypes as C

import numpy as np

from ._packed import device_records, points as _points

COUNTS = ("repeat", "extra", "max_back", "max_back_point", "seen", "history", "refuted", "truncated")
RULES = {"positional": 0, "situational": 1}
REPEAT, EXTRA, LEGAL = 0, 1, 2


def rule_of(rule):
    """0 / 1 of a rule given by number or by name"""
    if rule in (0, 1):
        return int(rule)
    if rule in RULES:
        return RULES[rule]
    raise ValueError("superko rule is 0 / 'positional' or 1 / 'situational', not %r" % (rule,))


class Superko(object):
    """sets uint32 [n, 3, NW] (repeat, extra, legal_superko), back int16 [n, N], counts int32 [n, 8] (COUNTS)."""

    def __init__(self, size, sets, back, counts):
        self.S, self.N = size, size * size
        self.sets, self.back = np.asarray(sets, dtype=np.uint32), np.asarray(back, dtype=np.int16)
        self.counts = np.asarray(counts, dtype=np.int32)

    def __len__(self):
        return len(self.counts)

    def count(self, i, name):
        return int(self.counts[i, COUNTS.index(name)])

    def repeat(self, i):
        """[(a, back)] of the empty points of row i whose ply repeats an earlier position, ascending"""
        return [(a, int(self.back[i, a])) for a in _points(self.sets[i, REPEAT], self.N)]

    def extra(self, i):
        """[(a, back)] of the repeating points the record's own legal set allows: what superko adds to the inherited rule"""
        return [(a, int(self.back[i, a])) for a in _points(self.sets[i, EXTRA], self.N)]

    def legal(self, i):
        """bool [N + 1]: the legal set without the repeating points; the pass is always legal"""
        bits = np.unpackbits(np.ascontiguousarray(self.sets[i, LEGAL], dtype="<u4").view(np.uint8), bitorder="little")
        return bits[:self.N + 1].astype(bool)

    def mask(self, i, which=REPEAT):
        """bool [N] of one of the sets of row i"""
        bits = np.unpackbits(np.ascontiguousarray(self.sets[i, which], dtype="<u4").view(np.uint8), bitorder="little")
        return bits[:self.N].astype(bool)

    def played(self, i, action):
        """(in repeat, in extra, back) of a played action in the position of row i; a pass repeats nothing"""
        if not 0 <= action < self.N:
            return False, False, -1
        return bool(self.mask(i, REPEAT)[action]), bool(self.mask(i, EXTRA)[action]), int(self.back[i, action])


def superko_dev(size, records, idx, first, rule, lib, rec_ptr=None, n_records=None):
    """sgo_superko_dev on device tensors: (sets int32 [n, 3, NW], back int16 [n, N], counts int32 [n, 8]) on the device; idx None:
    every record in order.  The work array of the keys is allocated here, one word per record."""
    import torch
    from . import _lib
    R = int(records.shape[0]) if n_records is None else int(n_records)
    n = int(first.shape[0])
    assert idx is None or int(idx.shape[0]) == n
    dev = records.device
    # the kernel writes every word of every row (the zero row for a row that names no history): nothing to clear first
    sets = torch.empty((n, 3, lib.sgo_plane_words(size)), dtype=torch.int32, device=dev)
    back = torch.empty((n, size * size), dtype=torch.int16, device=dev)
    counts = torch.empty((n, 8), dtype=torch.int32, device=dev)
    keys = torch.empty(max(R, 1), dtype=torch.int64, device=dev)
    _lib.check(lib.sgo_superko_dev(C.c_int(size), C.c_int(n), C.c_void_p(rec_ptr) if rec_ptr is not None else _lib.ptr(records), C.c_int(R),
                                   _lib.ptr(idx), _lib.ptr(first), C.c_int(rule_of(rule)), _lib.ptr(keys), _lib.ptr(sets), _lib.ptr(back),
                                   _lib.ptr(counts), _lib.stream_ptr()), "sgo_superko_dev")
    return sets, back, counts


def superko(size, records, index, first, rule=0):
    """sgo_superko_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Superko with one row per
    entry of `first` -- record index[i] (index None: record i) with the history first[i] .. index[i].  A row whose record is
    outside [0, R), or whose first is negative or behind it, gives the zero row."""
    import torch
    from . import _lib
    records, R, idx, _ = device_records(size, records, index)
    d_first = torch.from_numpy(np.ascontiguousarray(first, np.int32)).to(records.device)
    if idx is None and int(d_first.shape[0]) != R:
        raise ValueError("superko: without an index there is one `first` per record")
    sets, back, counts = superko_dev(size, records, idx, d_first, rule, _lib.load())
    return Superko(size, sets.cpu().numpy().view(np.uint32), back.cpu().numpy(), counts.cpu().numpy())


def format_repeat(v, i, vertex):
    """`sgo-superko` text of row i of a Superko: one line `V back` per repeating point, ascending, with `forbidden` appended where
    the inherited rule would allow the move (the point is in extra)"""
    extra = {a for a, _ in v.extra(i)}
    return "\n".join("%s %d%s" % (vertex(a), b, " forbidden" if a in extra else "") for a, b in v.repeat(i))


# ---- game review ---------------------------------------------------------------------------------------------------------------------
def review_flags(v, i, action, vertex=str):
    """Flags of one played move from row i of a Superko (the position BEFORE the move): `repeats K` when the move was in repeat,
    K = its back (the position it recreated stands K records before the one it was played from: 1 for a ko recapture);
    `superko-forbidden V ...` with the points of extra, whatever was played."""
    flags = []
    rep, _, back = v.played(i, action)
    if rep:
        flags.append("repeats %d" % back)
    extra = v.extra(i)
    if extra:
        flags.append("superko-forbidden " + " ".join(vertex(a) for a, _ in extra))
    return flags


# ---- record statistics ---------------------------------------------------------------------------------------------------------------
def game_report(name, v, base, played, actions):
    """What `records --superko` says of one game whose records are rows base .. base + played of v and whose entries are `actions`
    (entry j stands between rows base + j and base + j + 1): {"name", "cycled_at" (the first ply -- 1-based, the number of the move
    that reached it -- whose position had been seen before and was not reached by a pass; None), "cycled_back", "through": [{"ply",
    "action", "back"}] the played moves that were in extra (repetitions the ko approximation let through), "ko_recaptures": the
    played moves that were in repeat but not legal}"""
    N = v.N
    out = {"name": name, "cycled_at": None, "cycled_back": 0, "through": [], "ko_recaptures": 0}
    for j in range(played):
        a = int(actions[j])
        rep, ext, back = v.played(base + j, a)
        if ext:
            out["through"].append({"ply": j + 1, "action": a, "back": back})
        elif rep:
            out["ko_recaptures"] += 1
        seen = v.count(base + j + 1, "seen")
        if out["cycled_at"] is None and seen > 0 and 0 <= a < N:
            out["cycled_at"], out["cycled_back"] = j + 1, seen
    return out


def bucket_table(ply, extra_counts, width=20):
    """[{"from", "to", "positions", "with_extra", "share"}] per bucket of `width` plies: the share of the positions whose extra is
    not empty.  ply int [n] (0-based), extra_counts int [n] (counts[:, 1])."""
    ply, extra_counts = np.asarray(ply, np.int64), np.asarray(extra_counts, np.int64)
    out = []
    for b in sorted(set((ply // width).tolist())):
        sel = (ply // width) == b
        k, hit = int(sel.sum()), int((extra_counts[sel] > 0).sum())
        out.append({"from": int(b * width + 1), "to": int((b + 1) * width), "positions": k, "with_extra": hit, "share": float(hit) / k if k else 0.0})
    return out


def format_report(games, table, vertex):
    lines = []
    for g in games:
        if g["cycled_at"] is not None:
            lines.append("%s: cycled at move %d (%d plies back)" % (g["name"], g["cycled_at"], g["cycled_back"]))
        for t in g["through"]:
            lines.append("%s: move %d %s repeats a position, back %d" % (g["name"], t["ply"], vertex(t["action"]), t["back"]))
    lines.append("games %d  cycled %d  repetitions played through %d  ko recaptures played through %d" % (
        len(games), sum(g["cycled_at"] is not None for g in games), sum(len(g["through"]) for g in games), sum(g["ko_recaptures"] for g in games)))
    lines.append("moves      positions  with-extra   share")
    for r in table:
        lines.append("%4d-%-4d  %9d  %10d  %6.3f" % (r["from"], r["to"], r["positions"], r["with_extra"], r["share"]))
    return "\n".join(lines)
