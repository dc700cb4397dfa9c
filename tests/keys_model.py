"""CPU model of the position keys (include/sgo.h "position keys"), written from the header's text on top of oracle.sym_lut only.
No code of the package takes part.  Everything is integer: the GPU results must match bit for bit.

FAULT SWITCHES -- each the kind of slip k_keys could hold (tests/test_keys_model_power.py shows that the cases of the GPU test
notice them).  Model and test helper only; no library code reads them.
  flag_as_stone   the to-play bit is hashed as a black point
  no_turn         the to-play word is left out
  signed_min      the minimum is taken over signed values
  first_k_only    canon_action is taken from the lowest k of the mask, not the minimum over the mask
  history_read    planes 2 / 3 are OR-ed into the stones
  padding_read    bits >= N (other than the flag) are counted as stones
  lut_inverse     L_k is replaced by its inverse (differs for k = 4 and 6)
  pass_moved      a pass is not kept at N"""
import functools

import numpy as np

from oracle import oracle

FAULTS = ("flag_as_stone", "no_turn", "signed_min", "first_k_only", "history_read", "padding_read", "lut_inverse", "pass_moved")
SIZES = (5, 7, 9, 13, 19)
M64 = (1 << 64) - 1


def sm(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def z(S, c, a):
    return sm((S << 24) | (c << 16) | a)


@functools.lru_cache(maxsize=None)
def luts(S, inverse=False):
    """int64 [8, A]: L_k = oracle.sym_lut(S, k), or its inverse"""
    out = np.stack([oracle.sym_lut(S, k).astype(np.int64) for k in range(8)])
    if inverse:
        inv = np.empty_like(out)
        for k in range(8):
            inv[k, out[k]] = np.arange(S * S + 1)
        return inv
    return out


@functools.lru_cache(maxsize=None)
def _tables(S, inverse):
    """uint64 [2, 8, 32 * NW]: z(S, c, L_k[a]); a >= N (read by the padding faults only) maps to itself"""
    N, NW = S * S, (S * S + 31) // 32
    L = luts(S, inverse)
    t = np.zeros((2, 8, 32 * NW), np.uint64)
    for c in range(2):
        for k in range(8):
            for a in range(32 * NW):
                t[c, k, a] = z(S, c, int(L[k, a]) if a < N else a)
    return t


def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").astype(bool)


def record_keys(S, rec, fault=None):
    """[key_0 .. key_7] (Python ints) of one record uint32 [16 * NW]"""
    N, NW = S * S, (S * S + 31) // 32
    rec = np.asarray(rec, dtype=np.uint32).reshape(16, NW)
    black, white = _bits(rec[0]), _bits(rec[1])
    w = bool(black[32 * NW - 1])
    if fault == "history_read":
        black, white = black | _bits(rec[2]), white | _bits(rec[3])
    keep = np.zeros(32 * NW, bool)
    keep[:N] = True
    kb, kw = keep.copy(), keep.copy()
    if fault == "padding_read":
        kb[:], kw[:] = True, True
        kb[32 * NW - 1] = False
    if fault == "flag_as_stone":
        kb[32 * NW - 1] = True
    black, white = black & kb, white & kw
    t = _tables(S, fault == "lut_inverse")
    turn = z(S, 2, 0) if (w and fault != "no_turn") else 0
    out = []
    for k in range(8):
        v = int(np.bitwise_xor.reduce(t[0, k][black])) if black.any() else 0
        v ^= int(np.bitwise_xor.reduce(t[1, k][white])) if white.any() else 0
        out.append(v ^ turn)
    return out


def outputs(S, key, t, fault=None):
    """(key0, canon, mask, canon_action) from the eight keys and a target (None: no target, action -1)"""
    N = S * S
    if fault == "signed_min":
        canon = min(key, key=lambda v: v - (1 << 64) if v >> 63 else v)
    else:
        canon = min(key)
    ks = [k for k in range(8) if key[k] == canon]
    mask = sum(1 << k for k in ks)
    L = luts(S, fault == "lut_inverse")
    action = -1
    if t is not None and 0 <= t <= N:
        if t == N and fault == "pass_moved":
            action = -1
        elif fault == "first_k_only":
            action = int(L[ks[0], t])
        else:
            action = min(int(L[k, t]) for k in ks)
    return key[0], canon, mask, action


def keys(S, records, index=None, target=None, fault=None):
    """The outputs of sgo_keys_dev for n rows: {"key0", "canon" uint64 [n], "mask", "canon_action" int32 [n]} (canon_action all -1
    without targets).  records uint32 [R, 16 * NW]; index None = rows 0 .. R - 1; a row outside [0, R) gives the zero row."""
    records = np.asarray(records, dtype=np.uint32)
    R = len(records)
    index = np.arange(R) if index is None else np.asarray(index, dtype=np.int64)
    n = len(index)
    out = {"key0": np.zeros(n, np.uint64), "canon": np.zeros(n, np.uint64), "mask": np.zeros(n, np.int32),
           "canon_action": np.full(n, -1, np.int32)}
    cache = {}
    for i, r in enumerate(index):
        r = int(r)
        if r < 0 or r >= R:
            continue
        if r not in cache:
            cache[r] = record_keys(S, records[r], fault)
        k0, canon, mask, action = outputs(S, cache[r], None if target is None else int(target[i]), fault)
        out["key0"][i], out["canon"][i], out["mask"][i], out["canon_action"][i] = k0, canon, mask, action
    return out


# ---- records from stone lists; the case set -----------------------------------------------------------------------------------
def build_record(S, black, white, white_to_play, rng=None):
    """uint32 [16 * NW].  With rng: a random pattern in planes 2..15 and in the padding bits of planes 0 / 1 (the flag is set as
    asked)."""
    N, NW = S * S, (S * S + 31) // 32
    rec = np.zeros((16, NW), np.uint32)
    if rng is not None:
        rec[:] = rng.randint(0, 1 << 32, size=(16, NW), dtype=np.uint64).astype(np.uint32)
        live = np.zeros(32 * NW, bool)
        live[:N] = True
        livew = np.packbits(live, bitorder="little").view("<u4").astype(np.uint32)
        rec[0] &= ~livew
        rec[1] &= ~livew
        rec[0, NW - 1] &= np.uint32(0x7fffffff)
    for plane, pts in ((0, black), (1, white)):
        for a in pts:
            rec[plane, a >> 5] |= np.uint32(1 << (a & 31))
    if white_to_play:
        rec[0, NW - 1] |= np.uint32(0x80000000)
    return rec.reshape(-1)


def moved(S, g, pts):
    """the points moved by table g"""
    L = luts(S)
    return sorted(int(L[g, a]) for a in pts)


SUBGROUPS = {"k1": (0, 1), "k2": (0, 2), "k3": (0, 3), "k5": (0, 5), "k7": (0, 7), "rot": (0, 4, 5, 6), "axes": (0, 2, 3, 5),
             "diagonals": (0, 1, 5, 7), "all": tuple(range(8))}


def case_positions(S):
    """[(name, black points, white points, order of the symmetry group the position is built to have)]"""
    N, m = S * S, S - 1
    P = lambda x, y: y * S + x                                                           # noqa: E731
    out = [("empty", [], [], 8)]
    for y in range((S + 1) // 2):                                                        # one point per symmetry class
        for x in range(y + 1):
            order = 8 if (x == y and 2 * x == m) else (2 if (x == y or 2 * y == m) else 1)
            out.append(("stone_%d_%d" % (x, y), [P(x, y)], [], order))
            out.append(("wstone_%d_%d" % (x, y), [], [P(x, y)], order))
    seed_b, seed_w = [P(0, 1), P(1, 3)], [P(2, 1), P(1, 0)]
    for name, H in sorted(SUBGROUPS.items()):
        b = sorted({a for g in H for a in moved(S, g, seed_b)})
        w = sorted({a for g in H for a in moved(S, g, seed_w)} - set(b))
        for g in (0, 1, 4):                                                              # the position and two of its images
            out.append(("inv_%s_g%d" % (name, g), moved(S, g, b), moved(S, g, w), len(H)))
    out.append(("corners", [P(0, 0), P(m, 0), P(0, m), P(m, m)], [P(m // 2, m // 2)], 8))
    out.append(("full_black", list(range(N)), [], 8))
    out.append(("last_row", [P(x, m) for x in range(S)], [P(x, 0) for x in range(0, S, 2)], 2))
    return out


def golden_records(S, limit=12):
    """packed records of positions the reference's random games reached (tests/golden/rules_S*.npz), history planes included"""
    from tests import rollout_model as rm
    from tests.helpers import load
    zf = load("rules_S%d.npz" % S)
    boards = np.concatenate([zf["g%02d_fulls" % g].astype(np.int32) for g in range(int(zf["n_games"]))])
    return rm.pack_boards(boards[:limit])


def case_records(S, seed=0):
    """(names, records uint32 [n, 16 * NW]): every constructed position for both sides to move over a random pattern, then the
    golden positions"""
    rng = np.random.RandomState(1000 * S + seed)
    names, recs = [], []
    for name, b, w, _ in case_positions(S):
        for wtp in (False, True):
            names.append("%s_%s" % (name, "w" if wtp else "b"))
            recs.append(build_record(S, b, w, wtp, rng))
    g = golden_records(S)
    names += ["golden_%d" % i for i in range(len(g))]
    return names, np.concatenate([np.stack(recs), g])


def case_rows(S, names, n_records):
    """(index, target) int32: every record with one target walking over -1 .. N + 1, then every symmetric constructed position with
    EVERY target of -1 .. N + 1 (where the minimum over the mask is not the lowest k's)."""
    N = S * S
    index = list(range(n_records))
    target = [i % (N + 3) - 1 for i in range(n_records)]
    for r, name in enumerate(names):
        if name.startswith(("inv_", "corners", "empty", "stone_0_0", "last_row")) and name.endswith("_w"):
            index += [r] * (N + 3)
            target += list(range(-1, N + 2))
    return np.array(index, np.int32), np.array(target, np.int32)
