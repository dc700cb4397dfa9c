"""CPU model of the influence map (include/sgo.h "influence"), written from the header's text on plain Python lists: one value per
point, neighbours by coordinates, one function (`bouzy`) for the whole schedule.  No code of the package takes part, and nothing
of the kernel's form (row masks, sign bits crossing lanes, on-board masks) is used.  Everything is integer: the GPU results must
match word for word.

FAULT SWITCHES -- each the kind of slip a kernel could hold (tests/test_influence_model_power.py shows which named case of
tests/influence_cases.py notices which).  Model and test helper only; no library code reads them.
  offboard_erodes          off-board neighbours count as "<= 0" (and ">= 0") neighbours in erosion
  padding_rows             rows S .. 31 of a 32-row strip carry values (the map is run on the strip and cropped)
  column_wrap              column S - 1 is next to column 0 of the next row
  gauss_seidel             a step updates the map in place, point by point, instead of writing a new one
  dilate_ignores_opponent  dilation adds the friendly neighbours whether or not a hostile one is adjacent
  dilate_counts_zero       dilation adds the neighbours with v >= 0 (v <= 0), not v > 0 (v < 0)
  erode_opposite_only      erosion counts only the neighbours of the opposite sign, not the zeros
  erode_no_clamp           erosion does not stop at 0
  flag_as_stone            the to-play flag is read as a black stone (on the strip the plane words form; at 5x5 it lies two rows
                           under the board)
  dead_ignored             no stone is lifted
  dead_on_empty            a `dead` bit on an empty point puts a black stone there (live = black ^ dead)
  lifted_counted_live      a lifted stone is counted among the live stones of its colour
  lifted_not_territory     the point of a lifted stone is kept out of the territory and moyo sets
  moyo_late                the moyo checkpoint is taken one erosion step late (never past the last step)
  moyo_early               the moyo checkpoint is taken one erosion step early (never before the dilated map)
  moyo_zero_missed         with erode_moyo == 0 the checkpoint is never taken and the moyo sets show the final map
  territory_holds_stones   the sets are not cleared of the live stones"""
import functools

import numpy as np

FAULTS = ("offboard_erodes", "padding_rows", "column_wrap", "gauss_seidel", "dilate_ignores_opponent", "dilate_counts_zero",
          "erode_opposite_only", "erode_no_clamp", "flag_as_stone", "dead_ignored", "dead_on_empty", "lifted_counted_live",
          "lifted_not_territory", "moyo_late", "moyo_early", "moyo_zero_missed", "territory_holds_stones")
SIZES = (5, 7, 9, 13, 19)
MAX_DILATE, MAX_ERODE = 8, 31
TERRITORY, AREA = (5, 10, 21), (4, 0, 0)
TRIPLES = ((5, 10, 21), (4, 0, 0), (8, 31, 31), (0, 0, 0), (1, 0, 1))


@functools.lru_cache(maxsize=None)
def neighbour_table(S, H, wrap=False):
    """per point of an S wide, H high board the tuple of its on-board 4-neighbours"""
    out = []
    for a in range(S * H):
        x, y = a % S, a // S
        ns = [(y + dy) * S + x + dx for dx, dy in ((0, -1), (0, 1), (-1, 0), (1, 0)) if 0 <= x + dx < S and 0 <= y + dy < H]
        if wrap:   # the points a - 1 and a + 1 of the flat array, whatever row they lie in
            ns = [b for b in (a - S, a + S, a - 1, a + 1) if 0 <= b < S * H]
        out.append(tuple(ns))
    return tuple(out)


def bouzy(S, black, white, dead=(), dilate=5, erode_moyo=10, erode_terr=21, fault=None, flag=False):
    """The header's map from point lists.  {"values": [N], "sets": (terr_black, terr_white, moyo_black, moyo_white) as sorted point
    lists, "counts": the eight of the header}."""
    assert 0 <= dilate <= MAX_DILATE and 0 <= erode_moyo <= erode_terr <= MAX_ERODE
    N = S * S
    H = S
    if fault == "padding_rows":
        H = 32
    elif fault == "flag_as_stone" and flag:
        H = (32 * ((N + 31) // 32) + S - 1) // S              # the strip that holds the flag's bit
    black, white = {a for a in black if a < N}, {a for a in white if a < N}
    white -= black                                            # a point in both planes is read as a black stone
    lifted = {a for a in dead if a < N and (a in black or a in white)}
    if fault == "dead_ignored":
        lifted = set()
    live_b, live_w = black - lifted, white - lifted
    if fault == "dead_on_empty":
        live_b |= {a for a in dead if a < N and a not in black and a not in white}
    if fault == "flag_as_stone" and flag:
        live_b = live_b | {32 * ((N + 31) // 32) - 1}
    nb = neighbour_table(S, H, fault == "column_wrap")
    v = [128 if a in live_b else -128 if a in live_w else 0 for a in range(S * H)]
    in_place = fault == "gauss_seidel"

    for _ in range(dilate):
        new = v if in_place else list(v)
        for a, ns in enumerate(nb):
            x, pos, neg, zero = v[a], 0, 0, 0
            for b in ns:
                y = v[b]
                if y > 0:
                    pos += 1
                elif y < 0:
                    neg += 1
                else:
                    zero += 1
            add_p, add_n = (pos + zero, neg + zero) if fault == "dilate_counts_zero" else (pos, neg)
            if x >= 0 and (neg == 0 or fault == "dilate_ignores_opponent"):
                x += add_p
            if v[a] <= 0 and (pos == 0 or fault == "dilate_ignores_opponent"):
                x -= add_n
            new[a] = x
        v = new

    if fault == "moyo_late":
        at = min(erode_moyo + 1, erode_terr)
    elif fault == "moyo_early":
        at = max(erode_moyo - 1, 0)
    elif fault == "moyo_zero_missed" and erode_moyo == 0:
        at = erode_terr
    else:
        at = erode_moyo
    moyo = list(v) if at == 0 else None
    for step in range(erode_terr):
        new = v if in_place else list(v)
        for a, ns in enumerate(nb):
            x = v[a]
            if x == 0:
                continue
            away = 4 - len(ns) if fault == "offboard_erodes" else 0
            for b in ns:
                y = v[b]
                if fault == "erode_opposite_only":
                    away += (y < 0) if x > 0 else (y > 0)
                else:
                    away += (y <= 0) if x > 0 else (y >= 0)
            if fault == "erode_no_clamp":
                new[a] = x - away if x > 0 else x + away
            else:
                new[a] = max(0, x - away) if x > 0 else min(0, x + away)
        v = new
        if step + 1 == at:
            moyo = list(v)

    v, moyo = v[:N], moyo[:N]
    stones = set() if fault == "territory_holds_stones" else ((live_b | live_w) & set(range(N)))
    if fault == "lifted_not_territory":
        stones = stones | lifted
    sets = tuple(sorted(a for a in range(N) if a not in stones and (m[a] > 0 if colour > 0 else m[a] < 0))
                 for m in (v, moyo) for colour in (1, -1))
    n_b, n_w = len(live_b & set(range(N))), len(live_w)
    if fault == "lifted_counted_live":
        n_b, n_w = n_b + len(lifted & black), n_w + len(lifted & white)
    tb, tw = len(sets[0]), len(sets[1])
    counts = [tb, tw, len(sets[2]), len(sets[3]), n_b, n_w, N - n_b - n_w - tb - tw, (n_b + tb) - (n_w + tw)]
    return {"values": v, "sets": sets, "counts": counts}


def _bits(words):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little"))


def words_of(pts, NW):
    w = np.zeros(NW, np.uint32)
    for a in pts:
        w[a >> 5] |= np.uint32(1 << (a & 31))
    return w


def points_of(words, N):
    """the points a < N of a bitset"""
    return [int(a) for a in _bits(words) if a < N]


def record_stones(S, rec):
    """(black, white, flag) of a packed record: the points a < N of planes 0 / 1, and the to-play flag"""
    N, NW = S * S, (S * S + 31) // 32
    p = np.asarray(rec, dtype=np.uint32).reshape(16, NW)
    return points_of(p[0], N), points_of(p[1], N), bool(p[0, NW - 1] >> 31)


def influence(S, records, index=None, dead=None, dilate=5, erode_moyo=10, erode_terr=21, fault=None):
    """The outputs of sgo_influence_dev for n rows: {"values" int16 [n, N], "sets" uint32 [n, 4, NW], "counts" int32 [n, 8]}.
    records uint32 [R, 16 * NW]; index None = rows 0 .. R - 1; dead None or uint32 [n, NW] per ROW; a row whose record index is
    outside [0, R) gives zeros."""
    records = np.asarray(records, dtype=np.uint32)
    R, N, NW = len(records), S * S, (S * S + 31) // 32
    index = np.arange(R) if index is None else np.asarray(index, dtype=np.int64)
    n = len(index)
    out = {"values": np.zeros((n, N), np.int16), "sets": np.zeros((n, 4, NW), np.uint32), "counts": np.zeros((n, 8), np.int32)}
    for i, r in enumerate(index):
        r = int(r)
        if r < 0 or r >= R:
            continue
        black, white, flag = record_stones(S, records[r])
        lift = [] if dead is None else [int(a) for a in _bits(np.asarray(dead, np.uint32)[i])]
        m = bouzy(S, black, white, lift, dilate, erode_moyo, erode_terr, fault, flag)
        out["values"][i] = m["values"]
        out["sets"][i] = np.stack([words_of(s, NW) for s in m["sets"]])
        out["counts"][i] = m["counts"]
    return out
