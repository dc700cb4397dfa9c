"""Influence and territory estimate on the device (include/sgo.h "influence", csrc/sgo_influence.hip): per position Bouzy's
dilation / erosion map of the stones, the territory and moyo it shows, and an area-score estimate.  An ESTIMATE, not a proof: the
heuristic counterpart of life.py, for the long stretch of a game in which nothing is proved yet.  No net, no search.

    from sejonggo_amd.influence import influence, PRESETS
    v = influence(19, records)                               # packed records uint32 [R, 16 * NW], host or device
    v.values[0], v.territory(0, +1), v.moyo(0, -1), v.margin(0), v.neutral(0), v.estimate(0, komi=7.5)
    influence(19, records, **PRESETS["area"])                # (4, 0, 0): who is nearer, point by point

records.RecordSet.influence() reads every position of a game collection, engine.SessionEngine.influence(slots) the positions of
session slots; GTP's `sgo-influence` / `sgo-estimate`, `python -m sejonggo_amd.review --influence` and `python -m
sejonggo_amd.records --influence` stand on them."""
import ctypes as C

import numpy as np

from ._packed import device_records, points as _points

MAX_DILATE, MAX_ERODE = 8, 31
# the classical triples: territory / moyo at (5, 10, 21), area at (4, 0, 0)
PRESETS = {"territory": {"dilate": 5, "erode_moyo": 10, "erode_terr": 21}, "area": {"dilate": 4, "erode_moyo": 0, "erode_terr": 0}}


def check_params(dilate, erode_moyo, erode_terr):
    """the header's refusals, before anything reaches the device"""
    for v in (dilate, erode_moyo, erode_terr):
        if int(v) != v:
            raise ValueError("influence: the step counts are integers")
    if not 0 <= dilate <= MAX_DILATE:
        raise ValueError("influence: dilate outside [0, %d]" % MAX_DILATE)
    if not (0 <= erode_moyo <= MAX_ERODE and 0 <= erode_terr <= MAX_ERODE):
        raise ValueError("influence: an erosion count outside [0, %d]" % MAX_ERODE)
    if erode_moyo > erode_terr:
        raise ValueError("influence: erode_moyo > erode_terr")
    return int(dilate), int(erode_moyo), int(erode_terr)


class Influence(object):
    """values int16 [n, N] (the territory map), sets uint32 [n, 4, NW] (terr_black, terr_white, moyo_black, moyo_white), counts
    int32 [n, 8] (|terr_black|, |terr_white|, |moyo_black|, |moyo_white|, live black, live white, neutral, margin).  colour: +1
    black, -1 white."""

    def __init__(self, size, values, sets, counts, status=None):
        self.S, self.N = size, size * size
        self.values = np.asarray(values, dtype=np.int16)
        self.sets, self.counts = np.asarray(sets, dtype=np.uint32), np.asarray(counts, dtype=np.int32)
        self.status = status

    def __len__(self):
        return len(self.counts)

    def territory(self, i, colour):
        """the points without a live stone that the territory map gives the colour"""
        return _points(self.sets[i, 0 if colour > 0 else 1], self.N)

    def moyo(self, i, colour):
        """the same in the moyo map; the territory lies inside it"""
        return _points(self.sets[i, 2 if colour > 0 else 3], self.N)

    def live(self, i, colour):
        """the number of the colour's stones that were not lifted"""
        return int(self.counts[i, 4 if colour > 0 else 5])

    def neutral(self, i):
        """points that are neither a live stone nor territory"""
        return int(self.counts[i, 6])

    def margin(self, i):
        """(live black + black territory) - (live white + white territory): the area-score estimate before komi"""
        return int(self.counts[i, 7])

    def estimate(self, i, komi=0.0):
        """margin - komi: positive = black ahead"""
        return self.margin(i) - float(komi)


def influence(size, records, index=None, dead=None, dilate=5, erode_moyo=10, erode_terr=21):
    """sgo_influence_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): an Influence with one row
    per entry of `index` (None: every record in order); an index outside [0, R) gives the zero row.  dead: None, or uint32
    [n, NW] per ROW (host or device) -- the stones to lift."""
    dilate, erode_moyo, erode_terr = check_params(dilate, erode_moyo, erode_terr)
    from . import _lib
    records, _, idx, n = device_records(size, records, index, error=lambda text: ValueError("influence: " + text))
    values, sets, counts = influence_dev(size, records, idx, n, dead, dilate, erode_moyo, erode_terr, _lib.load())
    return Influence(size, values.cpu().numpy(), sets.cpu().numpy().view(np.uint32), counts.cpu().numpy())


def influence_dev(size, records, idx, n, dead, dilate, erode_moyo, erode_terr, lib, rec_ptr=None, n_records=None):
    """the launch on device tensors: (values int16 [n, N], sets int32 [n, 4, NW] holding the uint32 bit patterns, counts int32
    [n, 8]) on the device of `records`"""
    import torch
    from . import _lib
    dev = records.device
    NW = lib.sgo_plane_words(size)
    if dead is not None:
        if not torch.is_tensor(dead):
            dead = torch.from_numpy(np.ascontiguousarray(dead, np.uint32).view(np.int32))
        dead = dead.to(dev, torch.int32).contiguous()
        if tuple(dead.shape) != (n, NW):
            raise ValueError("influence: dead must be [n, NW] words, one row per listed row")
    values = torch.zeros((n, size * size), dtype=torch.int16, device=dev)
    sets = torch.zeros((n, 4, NW), dtype=torch.int32, device=dev)
    counts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    if n:
        _lib.check(lib.sgo_influence_dev(C.c_int(size), C.c_int(n), C.c_void_p(rec_ptr) if rec_ptr is not None else _lib.ptr(records),
                                         C.c_int(int(records.shape[0]) if n_records is None else n_records), _lib.ptr(idx), _lib.ptr(dead),
                                         C.c_int(dilate), C.c_int(erode_moyo), C.c_int(erode_terr), _lib.ptr(values), _lib.ptr(sets),
                                         _lib.ptr(counts), _lib.stream_ptr()), "sgo_influence_dev")
    return values, sets, counts


def dead_from_life(life_sets, black, white):
    """The stones sgo_life_dev proves dead, as the `dead` rows of the same positions: white stones in terr_black and black stones in
    terr_white.  life_sets [n, 4, NW] (alive_black, alive_white, terr_black, terr_white), black / white [n, NW] the stone planes;
    numpy arrays or tensors alike (two mask operations)."""
    return (life_sets[:, 2] & white) | (life_sets[:, 3] & black)


# ---- text ------------------------------------------------------------------------------------------------------------------------
def score_text(x):
    """`B+x.x` / `W+x.x` / `0` of an estimate (positive = black)"""
    return "0" if x == 0 else "%s+%.1f" % ("B" if x > 0 else "W", abs(x))


def estimate_line(v, i=0, komi=0.0):
    """`estimate B+x.x black P white Q neutral R komi K`: black / white = live stones + territory"""
    c = v.counts[i]
    return "estimate %s black %d white %d neutral %d komi %.1f" % (score_text(v.estimate(i, komi)), int(c[4]) + int(c[0]),
                                                                  int(c[5]) + int(c[1]), int(c[6]), float(komi))


def format_board(v, stones, i=0, komi=0.0):
    """`sgo-influence` text of row i of an Influence: S lines of S characters from the top row down -- X / O a live black / white
    stone, b / w a point of black / white territory, + / - a point of black / white moyo beyond the territory, . neutral -- then
    the estimate line.  stones int8 [N] (+1 black, -1 white) of the position; a stone that lies in a territory set was lifted and
    is drawn as territory."""
    S, N = v.S, v.N
    text = ["."] * N
    for colour, mark in ((1, "+"), (-1, "-")):
        for a in v.moyo(i, colour):
            text[a] = mark
    for colour, mark in ((1, "b"), (-1, "w")):
        for a in v.territory(i, colour):
            text[a] = mark
    marked = set(v.moyo(i, 1)) | set(v.moyo(i, -1)) | set(v.territory(i, 1)) | set(v.territory(i, -1))
    for a in range(N):
        # a live stone lies in no set and keeps its sign; a lifted stone whose point stayed neutral is drawn as neutral
        if stones[a] and a not in marked and int(v.values[i, a]) * int(stones[a]) > 0:
            text[a] = "X" if stones[a] > 0 else "O"
    lines = ["".join(text[y * S:(y + 1) * S]) for y in range(S)]
    lines.append(estimate_line(v, i, komi))
    return "\n".join(lines)


# ---- game review: what the estimate says in front of every move, and what the move did to it ------------------------------------
def review_fields(v, before, after, colour, komi):
    """{"estimate", "gain"} of one move from the Influence rows of the position in front of it (`before`) and behind it
    (`after`; None when unknown): estimate = margin - komi in front of the move, gain = the change of the margin across the move in
    the mover's favour (colour +1 black, -1 white).  Numbers, not verdicts."""
    out = {"estimate": v.estimate(before, komi)}
    out["gain"] = None if after is None else int(colour) * (v.margin(after) - v.margin(before))
    return out


def review_summary(gains, top=3):
    """(best, worst): the `top` move numbers with the highest and with the lowest gain; gains = [(move number, gain or None)]"""
    known = [(g, n) for n, g in gains if g is not None]
    best = [n for g, n in sorted(known, key=lambda t: (-t[0], t[1]))[:top]]
    worst = [n for g, n in sorted(known, key=lambda t: (t[0], t[1]))[:top]]
    return best, worst
