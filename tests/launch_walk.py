"""A tiny model of a CAPPED LAUNCH: a kernel whose grid stops at a cap and whose workgroups walk the remaining rows in a stride
loop (k_keys, k_tactics_read, k_solve_read, k_race_read, k_rollout_start, k_secure of sejonggo_amd/csrc).  No code of the package
takes part.

A launch is (n rows, cap_rows rows per trip of the grid, rows_per_block rows per workgroup).  Trip k of workgroup b covers rows
k * cap_rows + b * rows_per_block + (0 .. rows_per_block - 1).  rows_of says, per output row, which trip writes it and which INPUT
row it is computed from; simulate turns that into an output array over an index list, the way the GPU tests read a launch: a row
is known by the record its index entry names (R for an entry out of range), an unwritten row keeps its fill.

FAULT SWITCHES -- each the kind of slip such a launch could hold (tests/test_launch_walk_power.py shows that the row counts and
the index lists of tests/test_gpu_capped_launches.py notice them).  Model and test helper only; no library code reads them.
  one_trip      rows at or above the cap are never written
  short_stride  the stride is one block short: the walk's counter advances by cap_rows - rows_per_block while the output row
                advances by cap_rows, so trip k computes row i from input row i - k * rows_per_block
  stale_trip    trip k > 0 computes from trip 0's input row, i % cap_rows
  tail_dropped  the last partial block of the last trip is skipped (rows_per_block > 1 and n no multiple of it; a launch of
                one-row blocks has no partial block and cannot hold this slip)
  lone_half     with two rows per wave, the odd last row is lost (an even rows_per_block and an odd n; a launch of one-row blocks
                cannot hold it)"""
import numpy as np

FAULTS = ("one_trip", "short_stride", "stale_trip", "tail_dropped", "lone_half")
EVERY = 4099                                                         # an entry out of range at every 4 099th position
FILL = -7                                                            # an unwritten row of simulate

# the launches of csrc as (cap_rows, rows_per_block) and the row counts the GPU tests give them
KEYS = {"cap_rows": 4096 * 8, "rows_per_block": 8, "n": 65547}       # launch_keys: 4 096 blocks of 8 half-waves
READER = {"cap_rows": 65535, "rows_per_block": 1, "n": 131072}       # k_tactics_read, k_solve_read, k_race_read: gridDim.y
START_CAP, START_BLOCK = 4096 * 256, 256                             # launch_start: one word or cell per thread
# k_rollout_start, (S, n_src, per_src, rows of the index list per trip of the record words: START_CAP / (RW * per_src) rounded)
START_CASES = {"a": (5, 43000, 1, 65536), "b": (5, 1031, 128, 512), "c": (19, 3001, 2, 2731)}


def applies(fault, rows_per_block):
    """can a launch of such blocks hold the slip at all?"""
    if fault == "tail_dropped":
        return rows_per_block > 1
    if fault == "lone_half":
        return rows_per_block % 2 == 0
    return True


def rows_of(n, cap_rows, rows_per_block, fault=None, first=0):
    """(trip int64 [n], src int64 [n]): the trip that writes output row i and the input row it is computed from; src -1 for a
    row that is never written (first > 0: the rows first .. n - 1 only, for a launch too long to lay out whole)"""
    assert n >= 0 and cap_rows >= rows_per_block >= 1 and cap_rows % rows_per_block == 0 and (fault is None or fault in FAULTS)
    i = np.arange(first, n, dtype=np.int64)
    trip = i // cap_rows
    src = i.copy()
    if fault == "one_trip":
        src[i >= cap_rows] = -1
    elif fault == "short_stride":
        src = i - trip * rows_per_block
    elif fault == "stale_trip":
        src = i % cap_rows
    elif fault == "tail_dropped":
        src[i >= n // rows_per_block * rows_per_block] = -1
    elif fault == "lone_half":
        if rows_per_block % 2 == 0 and n % 2 == 1:
            src[-1] = -1
    return trip, src


def out_of_range(R):
    return (-1, R, -2 ** 31, 2 ** 31 - 1)


def listed(R, cap_rows):
    """how many of the R records of a case set an index list names: R, or the largest number below it, where (cap_rows + 1) % R
    is 0 and wrapped_index would give a row and its twin one trip later the same record (the 32 tactics records at 5x5: 31)"""
    while R > 1 and (cap_rows + 1) % R == 0:
        R -= 1
    return R


def wrapped_index(n, cap_rows, R, with_out_of_range=True):
    """int32 [n]: index[i] = (i + i // cap_rows) % R, so that a row and its twin one trip later name different records (iff
    (cap_rows + 1) % R != 0), with an entry out of range (-1, R, -2**31, 2**31 - 1 in turn) at every 4 099th position COUNTED
    FROM THE LAST ROW: row n - 1 is one, so that a last trip of two rows holds one as well
    (with_out_of_range=False: none, for a list the ABI gives no out-of-range convention)"""
    i = np.arange(n, dtype=np.int64)
    index = (i + i // cap_rows) % R
    at = np.flatnonzero((n - 1 - i) % EVERY == 0) if with_out_of_range else np.zeros(0, np.int64)
    index[at] = np.array(out_of_range(R), np.int64)[np.arange(len(at)) % 4]
    return index.astype(np.int32)


def record_of(index, R):
    """int64 [n]: the record a row shows, R (the out-of-range row of a padded table) for an entry outside [0, R)"""
    index = np.asarray(index, dtype=np.int64)
    return np.where((index >= 0) & (index < R), index, R)


def simulate(n, index, R, cap_rows, rows_per_block, fault=None, pad=2):
    """int64 [n + pad]: what a launch leaves in an output pre-filled with FILL: the record each written row shows"""
    trip, src = rows_of(n, cap_rows, rows_per_block, fault)
    out = np.full(n + pad, FILL, np.int64)
    rec = record_of(index, R)
    w = src >= 0
    out[:n][w] = rec[src[w]]
    return out


START_SOURCES = 29


def start_positions(S):
    """[(black, white, white_to_play)] x START_SOURCES: one colour fills the board but for two to four one-point eyes that do not
    touch, the OTHER colour is to move and has no stone: each of its moves would be suicide, so it has no legal board point and a
    rollout from here passes whatever its policy row says.  The area score of such a position is the whole board for the wall."""
    rng = np.random.RandomState(31 * S)
    out = []
    for k in range(START_SOURCES):
        eyes = []
        while len(eyes) < 2 + k % 3:
            a = int(rng.randint(S * S))
            if all(abs(a % S - e % S) + abs(a // S - e // S) > 1 for e in eyes):
                eyes.append(a)
        wall = sorted(set(range(S * S)) - set(eyes))
        out.append((wall, [], True) if k % 2 == 0 else ([], wall, False))
    return out


def start_sources(S):
    """(records uint32 [START_SOURCES, 16 * NW] over random words in planes 4..15 and in the padding, owner int32 [START_SOURCES]:
    +1 where the wall is black)"""
    from tests import tactics_model as T
    rng = np.random.RandomState(37 * S)
    pos = start_positions(S)
    return np.stack([T.build_record(S, b, w, wtp, None, None, rng) for b, w, wtp in pos]), np.array([1 if b else -1 for b, w, wtp in pos], np.int32)


def start_words(S, n_src, per_src, index, R, fault=None):
    """k_rollout_start's record copy as a launch of one WORD per row: int64 [words + 2], word w of record r as r * RW + w; the
    input row of a word names the source through (row // RW) // per_src and the word through row % RW"""
    RW = 16 * ((S * S + 31) // 32)
    n = n_src * per_src * RW
    trip, src = rows_of(n, START_CAP, START_BLOCK, fault)
    out = np.full(n + 2, FILL, np.int64)
    rec = record_of(index, R)
    w = src >= 0
    out[:n][w] = rec[src[w] // RW // per_src] * RW + src[w] % RW
    return out


def start_cells(S, n_src, per_src, fault=None, top_from_words=False):
    """the ownership cells k_rollout_start zeroes in the same walk: bool [n_src * N], True where a cell is written.  Every cell
    gets the same zero, so only a cell that is NOT written can show.  top_from_words: the walk ends at the record words, without
    `top = max(words, own_n)`"""
    RW = 16 * ((S * S + 31) // 32)
    own_n, words = n_src * S * S, n_src * per_src * RW
    trip, src = rows_of(own_n, START_CAP, START_BLOCK, fault)
    done = src >= 0
    if top_from_words:
        done &= np.arange(own_n) < words
    return done


# ---- k_secure: one (row, pair of candidates) UNIT per workgroup ------------------------------------------------------------------
SECURE_CAP = 1 << 24                                                 # SECURE_GRID_CAP of csrc/sgo_secure.hip, in units
# (ch: the workgroups per row, forced to the pairs (S * S + 1) // 2 of a row through sgo_secure_mode; n: the rows the GPU test gives)
SECURE = {5: {"ch": 13, "n": 1296001}, 19: {"ch": 181, "n": 97999}}


def secure_geometry(S):
    """(ch, n, astride, first_whole, k0): unit SECURE_CAP is pair k0 of row `astride` -- its pairs below k0 belong to trip 0, the rest
    to trip 1 -- and `first_whole` = astride + 1 is the first row wholly in the second trip"""
    ch, n = SECURE[S]["ch"], SECURE[S]["n"]
    astride, k0 = SECURE_CAP // ch, SECURE_CAP % ch
    return ch, n, astride, astride + 1, k0


def secure_listed(R, first_whole):
    """how many of the R records of a case set the index list of the secure launch names: wrapped_index(n, first_whole, R) gives the
    rows from first_whole on the record (i + 1) % R and the units of such a row have their twins one trip earlier in the rows
    i - first_whole and i - first_whole + 1, those of the row astride the cap in row 0: R, or the largest number below it that
    divides none of first_whole - 1, first_whole and first_whole + 1 (the 76 securing cases at 5x5: 75)"""
    while R > 1 and any((first_whole + d) % R == 0 for d in (-1, 0, 1)):
        R -= 1
    return R


def secure_entries(S, index, R, fault=None, first=0):
    """k_secure's table as a launch of one UNIT per row of the model: int64 [(n - first) + 2, ch], entry (row i, pair k) -- the
    table rows of the (2k)-th and (2k + 1)-th empty point -- as record * ch + pair, written by unit i * ch + k % ch (ch = pairs: k);
    unit u is computed from the record that the index entry of row u // ch names.  The rows first .. n - 1 and two rows behind n."""
    ch, n = SECURE[S]["ch"], SECURE[S]["n"]
    trip, src = rows_of(n * ch, SECURE_CAP, 1, fault, first=first * ch)
    out = np.full((n - first + 2) * ch, FILL, np.int64)
    rec = record_of(index, R)
    w = src >= 0
    out[:(n - first) * ch][w] = rec[src[w] // ch] * ch + src[w] % ch
    return out.reshape(n - first + 2, ch)
