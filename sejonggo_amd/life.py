"""Unconditional life on the device (include/sgo.h "unconditional life", csrc/sgo_life.hip): per position the stones of either
colour that can never be captured whatever the opponent plays (Benson's pass-alive chains), the points they enclose, and how much
of the board is settled by them.  Proved, not estimated: no net, no search caps, no "unknown".

    from sejonggo_amd.life import life
    v = life(19, records)                    # packed records uint32 [R, 16 * NW], host or device
    v.alive(0, +1), v.territory(0, -1), v.dead(0, +1), v.unsettled(0), v.margin(0), v.settled(0)

records.RecordSet.life() reads every position of a game collection, engine.SessionEngine.life(slots) the positions of session
slots; GTP's `sgo-life`, `python -m sejonggo_amd.review --life` and `python -m sejonggo_amd.records --life` stand on them."""
import ctypes as C

import numpy as np

from ._packed import device_records, points as _points


class Life(object):
    """sets uint32 [n, 4, NW] (alive_black, alive_white, terr_black, terr_white), counts int32 [n, 8] (|alive_black|, |alive_white|,
    |terr_black|, |terr_white|, dead_white, dead_black, unsettled, margin).  colour: +1 black, -1 white."""

    def __init__(self, size, sets, counts):
        self.S, self.N = size, size * size
        self.sets, self.counts = np.asarray(sets, dtype=np.uint32), np.asarray(counts, dtype=np.int32)

    def __len__(self):
        return len(self.counts)

    def alive(self, i, colour):
        """the points of the colour's stones that can never be captured"""
        return _points(self.sets[i, 0 if colour > 0 else 1], self.N)

    def territory(self, i, colour):
        """the points (empty, or dead stones of the other colour) the colour's living chains enclose"""
        return _points(self.sets[i, 2 if colour > 0 else 3], self.N)

    def dead(self, i, colour, stones):
        """the colour's stones inside the other colour's territory; stones int8 [N] (+1 black, -1 white)"""
        return [a for a in self.territory(i, -colour) if stones[a] == colour]

    def n_dead(self, i, colour):
        return int(self.counts[i, 5 if colour > 0 else 4])

    def safe(self, i, colour):
        return sorted(self.alive(i, colour) + self.territory(i, colour))

    def unsettled(self, i):
        """points that belong to neither colour's living chains or their territory"""
        return int(self.counts[i, 6])

    def margin(self, i):
        """|safe_black| - |safe_white|"""
        return int(self.counts[i, 7])

    def settled(self, i):
        return self.unsettled(i) == 0


def life(size, records, index=None):
    """sgo_life_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Life with one row per entry
    of `index` (None: every record in order); an index outside [0, R) gives the zero row."""
    import torch
    from . import _lib
    records, R, idx, n = device_records(size, records, index)
    lib, dev = _lib.load(), records.device
    sets = torch.zeros((n, 4, lib.sgo_plane_words(size)), dtype=torch.int32, device=dev)
    counts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    _lib.check(lib.sgo_life_dev(C.c_int(size), C.c_int(n), _lib.ptr(records), C.c_int(R), _lib.ptr(idx), _lib.ptr(sets), _lib.ptr(counts),
                                _lib.stream_ptr()), "sgo_life_dev")
    return Life(size, sets.cpu().numpy().view(np.uint32), counts.cpu().numpy())


def format_board(v, i=0):
    """`sgo-life` text of row i of a Life: S lines of S characters from the top row down -- B / W an alive stone, b / w a point of
    black / white territory (empty, or a dead stone of the other colour), . anything else -- then `settled P/N black SB white SW`
    (P = the points that are safe for either colour, SB / SW = |safe_black| / |safe_white|)."""
    S, N = v.S, v.N
    text = ["."] * N
    for colour, stone, point in ((1, "B", "b"), (-1, "W", "w")):
        for a in v.alive(i, colour):
            text[a] = stone
        for a in v.territory(i, colour):
            text[a] = point
    c = v.counts[i]
    lines = ["".join(text[y * S:(y + 1) * S]) for y in range(S)]
    lines.append("settled %d/%d black %d white %d" % (N - int(c[6]), N, int(c[0]) + int(c[2]), int(c[1]) + int(c[3])))
    return "\n".join(lines)


# ---- game review: which moves were played inside settled territory, and when was the whole board decided ------------------------
def review_flags(size, action, v, before, already_decided):
    """Flags of one move from the Life row `before` of the position in front of it:
    `inside`   the move is played on a point that lay in terr_black | terr_white of that position;
    `decided`  that position has unsettled == 0 and no earlier one had (already_decided False).
    A pass is never `inside`."""
    flags = []
    if 0 <= action < size * size and (action in v.territory(before, 1) or action in v.territory(before, -1)):
        flags.append("inside")
    if v.settled(before) and not already_decided:
        flags.append("decided")
    return flags
