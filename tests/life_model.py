"""CPU model of unconditional life (include/sgo.h "unconditional life"), written from the header's text on plain Python sets of
points: chains and regions by breadth-first search, vitality by the definition, the removal loop as the header states it.  No code
of the package takes part, and nothing of the kernel's shortcuts (lowest empty point, row bitboards) is used.  Everything is
integer: the GPU results must match word for word.  It works on packed records for the supported sizes (`life`) and on point lists
for any S >= 3 (`benson`).

FAULT SWITCHES -- each the kind of slip a kernel could hold (tests/test_life_model_power.py shows which case notices which).
Model and test helper only; no library code reads them.
  one_vital_enough                a chain stays with one vital region
  some_empty_adjacent             a region is vital when ANY of its empty points touches the chain, not every one
  regions_not_removed             the regions next to a removed chain stay in the region set
  single_round                    the removal runs once and is not repeated
  all_kept_regions_are_territory  every region left is territory, vital to a living chain or not
  empty_less_region_vital         a region without an empty point is vital to the chains around it
  stones_must_be_adjacent         opponent stones in a region are treated like empty points: they too must touch the chain
  region_8_connected              regions are joined diagonally as well
  flag_as_stone                   the to-play flag is read as a black stone
  padding_read                    bits >= N of planes 0 / 1 (other than the flag) are read as stones

With flag_as_stone / padding_read the position is taken on the STRIP the plane words form (width S, 32 * NW points), as a kernel
reading the words without a mask would see it; the output words then carry what the strip holds.

The number of removal passes (`rounds`: the passes that removed something, plus the last one that did not) is internal to the
model: the interface does not expose it."""
import numpy as np

FAULTS = ("one_vital_enough", "some_empty_adjacent", "regions_not_removed", "single_round", "all_kept_regions_are_territory",
          "empty_less_region_vital", "stones_must_be_adjacent", "region_8_connected", "flag_as_stone", "padding_read")
SIZES = (5, 7, 9, 13, 19)
N4 = ((1, 0), (-1, 0), (0, 1), (0, -1))
N8 = N4 + ((1, 1), (1, -1), (-1, 1), (-1, -1))


def neighbours(S, a, area, steps=N4):
    """the points of [0, area) next to a on a board (or strip) S wide"""
    x, y = a % S, a // S
    out = []
    for dx, dy in steps:
        if 0 <= x + dx < S and y + dy >= 0:
            b = (y + dy) * S + x + dx
            if b < area:
                out.append(b)
    return out


def components(S, pts, area, steps=N4):
    """the maximal connected subsets of pts, each a frozenset, in ascending order of their lowest point"""
    pts, out = set(pts), []
    for a in sorted(pts):
        if a not in pts:
            continue
        comp, todo = {a}, [a]
        pts.discard(a)
        while todo:
            for b in neighbours(S, todo.pop(), area, steps):
                if b in pts:
                    pts.discard(b)
                    comp.add(b)
                    todo.append(b)
        out.append(frozenset(comp))
    return out


def benson(S, own, other, fault=None, area=None):
    """(alive, territory, rounds) of colour X = `own` against O = `other` (point lists or sets) on an S x S board (area None), or
    on the first `area` points of a strip S wide"""
    area = S * S if area is None else area
    own, other = set(own), set(other)
    every = set(range(area))
    empty = every - own - other
    chains = components(S, own, area)
    regions = components(S, every - own, area, N8 if fault == "region_8_connected" else N4)
    border = {c: frozenset(b for a in c for b in neighbours(S, a, area)) for c in chains}   # the points next to a chain

    def vital(r, c):
        need = r if fault == "stones_must_be_adjacent" else r & empty
        if not need:
            return fault == "empty_less_region_vital" and bool(r & border[c])
        if fault == "some_empty_adjacent":
            return bool(need & border[c])
        return need <= border[c]

    rounds = 0
    while True:
        rounds += 1
        least = 1 if fault == "one_vital_enough" else 2
        out = [c for c in chains if sum(vital(r, c) for r in regions) < least]
        if not out:
            break
        chains = [c for c in chains if c not in out]
        if fault != "regions_not_removed":
            touched = set().union(*[border[c] for c in out])
            regions = [r for r in regions if not r & touched]
        if fault == "single_round":
            break
    alive = set().union(*chains) if chains else set()
    terr = set()
    for r in regions:
        if fault == "all_kept_regions_are_territory" or any(vital(r, c) for c in chains):
            terr |= r
    return alive, terr, rounds


def _bits(words):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little"))


def record_stones(S, rec, fault=None):
    """(black, white, area): the stones of a packed record as point lists, and how many points the position has"""
    N, NW = S * S, (S * S + 31) // 32
    p = np.asarray(rec, dtype=np.uint32).reshape(16, NW)
    black, white = [int(a) for a in _bits(p[0])], [int(a) for a in _bits(p[1])]
    flag = 32 * NW - 1
    if fault == "padding_read":
        return [a for a in black if a != flag], [a for a in white if a not in black], 32 * NW
    if fault == "flag_as_stone":
        return [a for a in black if a < N or a == flag], [a for a in white if a < N], 32 * NW
    return [a for a in black if a < N], [a for a in white if a < N], N


def _words(pts, NW):
    w = np.zeros(NW, np.uint32)
    for a in pts:
        w[a >> 5] |= np.uint32(1 << (a & 31))
    return w


def point_life(S, black, white, fault=None, area=None):
    """{"alive": (black, white), "terr": (black, white), "rounds": (black, white), "counts": the eight of the header} from point
    lists, any S >= 3"""
    N = S * S
    ab, tb, rb = benson(S, black, white, fault, area)
    aw, tw, rw = benson(S, white, black, fault, area)
    sb, sw = ab | tb, aw | tw
    counts = [len(ab), len(aw), len(tb), len(tw), len(tb & set(white)), len(tw & set(black)), N - len(sb | sw), len(sb) - len(sw)]
    return {"alive": (ab, aw), "terr": (tb, tw), "rounds": (rb, rw), "counts": counts}


def record_life(S, rec, fault=None):
    """(sets uint32 [4, NW], counts int32 [8], rounds (black, white)) of one packed record"""
    NW = (S * S + 31) // 32
    black, white, area = record_stones(S, rec, fault)
    m = point_life(S, black, white, fault, area)
    sets = np.stack([_words(m["alive"][0], NW), _words(m["alive"][1], NW), _words(m["terr"][0], NW), _words(m["terr"][1], NW)])
    return sets, np.array(m["counts"], np.int32), m["rounds"]


def life(S, records, index=None, fault=None):
    """The outputs of sgo_life_dev for n rows: {"sets" uint32 [n, 4, NW], "counts" int32 [n, 8], "rounds" int32 [n, 2]}.  records
    uint32 [R, 16 * NW]; index None = rows 0 .. R - 1; a row outside [0, R) gives zero sets and counts."""
    records = np.asarray(records, dtype=np.uint32)
    R, NW = len(records), (S * S + 31) // 32
    index = np.arange(R) if index is None else np.asarray(index, dtype=np.int64)
    n = len(index)
    out = {"sets": np.zeros((n, 4, NW), np.uint32), "counts": np.zeros((n, 8), np.int32), "rounds": np.zeros((n, 2), np.int32)}
    cache = {}
    for i, r in enumerate(index):
        r = int(r)
        if r < 0 or r >= R:
            continue
        if r not in cache:
            cache[r] = record_life(S, records[r], fault)
        out["sets"][i], out["counts"][i], out["rounds"][i] = cache[r]
    return out


def build_record(S, black, white, white_to_play, rng=None):
    """uint32 [16 * NW]: planes 0 / 1 the stones.  With rng: random words in planes 2..15 and in the padding bits of planes 0 / 1
    (the flag is set as asked)."""
    N, NW = S * S, (S * S + 31) // 32
    rec = np.zeros((16, NW), np.uint32)
    if rng is not None:
        rec[:] = rng.randint(0, 1 << 32, size=(16, NW), dtype=np.uint64).astype(np.uint32)
        live = np.zeros(32 * NW, bool)
        live[:N] = True
        livew = np.packbits(live, bitorder="little").view("<u4").astype(np.uint32)
        rec[:2] &= ~livew
        rec[0, NW - 1] &= np.uint32(0x7fffffff)
    for plane, pts in enumerate((black, white)):
        for a in pts:
            rec[plane, a >> 5] |= np.uint32(1 << (a & 31))
    if white_to_play:
        rec[0, NW - 1] |= np.uint32(0x80000000)
    return rec.reshape(-1)


def points_of(words, N):
    """the points a < N of a bitset"""
    return [int(a) for a in _bits(words) if a < N]
