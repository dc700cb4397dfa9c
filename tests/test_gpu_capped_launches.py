"""GPU: every launch of csrc that caps its grid and walks the remaining rows in a stride loop, run PAST its cap and compared whole
with the existing models: k_keys (4 096 blocks of 8 rows), k_tactics_read, k_solve_read and k_race_read (gridDim.y = 65 535),
k_rollout_start (4 096 blocks of 256 words or ownership cells) and k_secure (1 << 24 workgroups of one pair of candidates each:
a ROW straddles the cap), then RecordSet.keys / RecordSet.tactics over a collection of more
than 2 * 65 535 positions in one chunk.  tests/launch_walk.py models such a launch; tests/test_launch_walk_power.py shows that
these row counts and index lists notice its fault switches.

Expected rows are the model's rows of the R records of a case set, computed once, laid out as one padded table per output (row R
the out-of-range row) and re-listed through the index; whole arrays are compared, the two pre-filled rows behind n included.

THE ROLLOUT SOURCES.  k_rollout_step never reads the pass entry of a policy row: a rollout passes only where its mover has no
legal board point.  So the sources are positions whose mover has none (launch_walk.start_positions; the oracle says so in
tests/test_launch_walk_power.py) and the run is one step under max_plies = 1: every rollout ends on its first ply, a pass, and the
ownership is the area score of the source -- no sampling model.  plies_sum = rollouts and capped = rollouts say that ply and passes
were zero when the step read them, also at the second start, which finds 1 and 1 there.

THE INDEX LISTS are launch_walk.wrapped_index: (i + i // cap_rows) % R with an entry out of range at every 4 099th position counted
from the last row.  A case set of 32 records (tactics at 5x5, races at 19x19) is listed without its last record, because 65 536 % 32
is 0 and the twin of a row one trip later would be the same record.

Measured on MI355X (pytest --durations=0 of this module within the whole suite, 16 tests, 6.3 s together):
  2.81s test_record_set_past_the_caps          0.76s test_tactics_three_trips[19]        0.09s test_tactics_three_trips[5]
  0.60s test_race_three_trips[19-enumerated]   0.32s test_race_three_trips[19-asked]     0.35s / 0.18s the same at 5x5
  0.41s test_solve_three_trips[19-asked]       0.37s test_solve_three_trips[19-enumerated]   0.07s / 0.05s the same at 5x5
  0.16s test_keys_three_trips[19]              0.09s / 0.01s / 0.01s test_rollout_start_walk[a / b / c]
  1.97s test_keys_three_trips[5] when the module runs alone (the first call of the process), 0.01s otherwise
test_secure_past_the_grid_cap, the two cases alone in a process: 1.98s at 5x5 and 4.37s at 19x19, of which 4.25s are the model's rows of
the 19x19 case set (computed once per process and shared with tests/test_gpu_secure.py); the two launches of sgo_secure_dev take
0.012s and 0.055s, the call with its fills and copies 0.1s, listing and comparing the table 0.1s"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import keys_model as K
from tests import launch_walk as W
from tests import race_cases as RC
from tests import race_model as RM
from tests import secure_cases as SEC
from tests import solve_cases as SC
from tests import solve_model as SM
from tests import tactics_cases as TC

pytestmark = pytest.mark.gpu

FILL32, FILL64 = 0x3C3C3C3C, 0x5A5A5A5A5A5A5A5A
SIZES = (5, 19)                                                      # the single-word and the 12-word plane instantiations
MAX_CHAINS, MAX_TARGETS, MAX_PAIRS = 4, 2, 2
SOLVE_NODES, RACE_NODES = 512, 512                                   # 131 072 rows are read; the model at the same cap decides all but two races


def _whole(got, want, what):
    """two whole arrays, rows behind n included; a difference names the first rows"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        raise AssertionError("%s: %d of %d rows differ, first %s; row %d is %s, the model's %s" % (
            what, len(bad), len(got), bad[:8].tolist(), bad[0], got[bad[0]].reshape(-1)[:16].tolist(), want[bad[0]].reshape(-1)[:16].tolist()))


def _listed(table, index, R, fill, pad=2):
    """a padded table [R + 1, ...] (row R: the out-of-range row) re-listed through an index, `pad` rows of `fill` behind it"""
    out = np.full((len(index) + pad,) + table.shape[1:], fill, table.dtype)
    out[:len(index)] = table[W.record_of(index, R)]
    return out


def _trips_differ(index, R, cap, *tables):
    """the expected rows themselves tell a row from its twin one trip later, on most rows"""
    a, b = W.record_of(index[:len(index) - cap], R), W.record_of(index[cap:], R)
    differ = np.zeros(len(a), bool)
    for t in tables:
        differ |= (t[a] != t[b]).reshape(len(a), -1).any(axis=1)
    return differ.mean()


def _padded(rows, T, width, fill, dtype):
    """a list of per-record arrays [k_r, width] as [R + 1, T, width]: the first T rows of each, `fill` behind them and in row R"""
    out = np.full((len(rows) + 1, T, width), fill, dtype)
    for r, a in enumerate(rows):
        k = min(len(a), T)
        out[r, :k] = a[:k]
    return out


# ---- keys ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _keys_tables(S):
    """(records [R], key0, canon uint64 [R + 1], mask int32 [R + 1], action int32 [R + 1, N + 3] by target + 1)"""
    N = S * S
    recs = K.case_records(S)[1]
    R = W.listed(len(recs), W.KEYS["cap_rows"])
    key0, canon = np.zeros(R + 1, np.uint64), np.zeros(R + 1, np.uint64)
    mask, action = np.zeros(R + 1, np.int32), np.full((R + 1, N + 3), -1, np.int32)
    for r in range(R):
        key = K.record_keys(S, recs[r])
        for t in range(-1, N + 2):
            key0[r], canon[r], mask[r], action[r, t + 1] = K.outputs(S, key, t)
    return recs[:R], key0, canon, mask, action


@pytest.mark.parametrize("S", SIZES)
def test_keys_three_trips(S):
    """n = 65 547: three trips of 4 096 blocks, the last block holding 3 of its 8 rows (and a lone half-wave); with and without a
    target list, in both sgo_keys_mode forms"""
    from sejonggo_amd import _lib as L
    from tests import test_gpu_keys as G
    lib = L.require_gpu()
    n, cap = W.KEYS["n"], W.KEYS["cap_rows"]
    recs, key0, canon, mask, action = _keys_tables(S)
    R = len(recs)
    index = W.wrapped_index(n, cap, R)
    target = (np.arange(n) % (S * S + 3) - 1).astype(np.int32)
    assert cap % (S * S + 3) != 0                                    # a row and its twin one trip later ask about different targets
    rec = W.record_of(index, R)
    want = {"key0": _listed(key0, index, R, FILL64), "canon": _listed(canon, index, R, FILL64), "mask": _listed(mask, index, R, G.FILL32)}
    act = np.full(n + 2, G.FILL32, np.int32)
    act[:n] = action[rec, target + 1]
    assert _trips_differ(index, R, cap, key0, canon) > 0.99 and (mask[:R] != 0).all() and len(np.unique(act[:n])) > S * S
    prev = lib.sgo_keys_mode(0)
    try:
        for mode in (0, 1):
            lib.sgo_keys_mode(mode)
            for tgt in (target, None):
                got = G._run(S, recs, index, tgt, pad=2)
                for k in ("key0", "canon", "mask"):
                    _whole(got[k], want[k], ("keys", S, mode, tgt is not None, k))
                _whole(got["canon_action"], act if tgt is not None else np.full(n + 2, G.FILL32, np.int32), ("keys", S, mode, tgt is not None, "action"))
    finally:
        lib.sgo_keys_mode(prev)


# ---- tactics ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tactics_tables(S):
    names, recs = TC.case_records(S)
    R = W.listed(len(recs), W.READER["cap_rows"])
    want = TC.case_model(S)
    libs = np.zeros((R + 1, S * S), np.uint8)
    libs[:R] = want["libs"][:R]
    n_chains = np.zeros(R + 1, np.int32)
    n_chains[:R] = want["n_chains"][:R]
    return names[:R], recs[:R], libs, n_chains, _padded(want["rows"][:R], MAX_CHAINS, 8, FILL32, np.int32)


@pytest.mark.parametrize("S", SIZES)
def test_tactics_three_trips(S):
    """n = 131 072: rows 131 070 and 131 071 are the third trip of k_tactics_read; max_chains = 4, so that records with more
    listed chains than rows (the lattice at 19x19) are among them"""
    from tests import test_gpu_tactics as G
    n, cap = W.READER["n"], W.READER["cap_rows"]
    names, recs, libs, n_chains, chains = _tactics_tables(S)
    R = len(recs)
    assert (n_chains > MAX_CHAINS).any() == (S == 19) and ("lattice_w" in names) == (S == 19) and (n_chains[:R] > 0).sum() > R // 2
    index = W.wrapped_index(n, cap, R)
    assert _trips_differ(index, R, cap, libs, n_chains, chains) > 0.8
    assert n_chains[index[n - 2]] >= MAX_CHAINS and index[n - 1] == 2 ** 31 - 1      # the third trip reads chains, beside a row out of range
    got = G._run(S, recs, index, max_chains=MAX_CHAINS, pad=2)
    _whole(got["n_chains"], _listed(n_chains, index, R, FILL32), ("tactics", S, "n_chains"))
    _whole(got["libs"], _listed(libs, index, R, G.FILL8), ("tactics", S, "libs"))
    _whole(got["chains"], _listed(chains, index, R, FILL32), ("tactics", S, "chains"))


# ---- solve --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solve_tables(S, asked):
    names, recs, ask, region, has = SC.case_records(S)
    R = W.listed(len(recs), W.READER["cap_rows"])
    NW = (S * S + 31) // 32
    want = SM.solve(S, recs[:R], ask=ask[:R] if asked else None, rules=1, max_region=SC.MAX_REGION, max_nodes=SOLVE_NODES, max_targets=MAX_TARGETS)
    n_targets = np.zeros(R + 1, np.int32)
    n_targets[:R] = want["n_targets"]
    return (recs[:R], ask[:R], n_targets, _padded(want["rows"], MAX_TARGETS, 8, FILL32, np.int32),
            _padded(want["regions"], MAX_TARGETS, NW, FILL32, np.uint32))


@pytest.mark.parametrize("asked", [True, False], ids=["asked", "enumerated"])
@pytest.mark.parametrize("S", SIZES)
def test_solve_three_trips(S, asked):
    """n = 131 072, max_targets = 2, the case set's max_region and rules = 1, max_nodes = 512 in the kernel and in the model"""
    from tests import test_gpu_solve as G
    n, cap = W.READER["n"], W.READER["cap_rows"]
    recs, ask, n_targets, rows, regions = _solve_tables(S, asked)
    R = len(recs)
    index = W.wrapped_index(n, cap, R)
    assert _trips_differ(index, R, cap, n_targets, rows, regions) > 0.4 and (n_targets > 0).sum() >= 4
    assert n_targets[index[n - 2]] > 0 or (S, asked) == (19, False)  # the third trip has a target to read (19x19 enumerated: none)
    got = G._run(S, recs, index, ask=ask[np.clip(index.astype(np.int64), 0, R - 1)] if asked else None, rules=1, max_region=SC.MAX_REGION,
                 max_nodes=SOLVE_NODES, max_targets=MAX_TARGETS, pad=2)
    _whole(got["n_targets"], _listed(n_targets, index, R, FILL32), ("solve", S, asked, "n_targets"))
    _whole(got["rows"], _listed(rows, index, R, FILL32), ("solve", S, asked, "rows"))
    _whole(got["regions"], _listed(regions, index, R, FILL32), ("solve", S, asked, "regions"))


# ---- race ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _race_tables(S, asked):
    names, recs, ask, region, has = RC.case_records(S)
    R = W.listed(len(recs), W.READER["cap_rows"])
    NW = (S * S + 31) // 32
    want = RM.race(S, recs[:R], ask=ask[:R] if asked else None, rules=1, max_libs=RC.MAX_LIBS, max_region=RC.MAX_REGION, max_nodes=RACE_NODES,
                   max_pairs=MAX_PAIRS)
    n_pairs = np.zeros(R + 1, np.int32)
    n_pairs[:R] = want["n_pairs"]
    return (recs[:R], ask[:R], n_pairs, _padded(want["rows"], MAX_PAIRS, 16, FILL32, np.int32),
            _padded(want["regions"], MAX_PAIRS, NW, FILL32, np.uint32))


@pytest.mark.parametrize("asked", [True, False], ids=["asked", "enumerated"])
@pytest.mark.parametrize("S", SIZES)
def test_race_three_trips(S, asked):
    """n = 131 072, max_pairs = 2, the case set's max_libs, max_region and rules = 1, max_nodes = 512 in the kernel and in the model"""
    from tests import test_gpu_race as G
    n, cap = W.READER["n"], W.READER["cap_rows"]
    recs, ask, n_pairs, rows, regions = _race_tables(S, asked)
    R = len(recs)
    index = W.wrapped_index(n, cap, R)
    assert _trips_differ(index, R, cap, n_pairs, rows, regions) > 0.4 and (n_pairs > 0).sum() > R // 2
    assert n_pairs[index[n - 2]] > 0                                 # the third trip has a pair to read
    got = G._run(S, recs, index, ask=ask[np.clip(index.astype(np.int64), 0, R - 1)] if asked else None, rules=1, max_libs=RC.MAX_LIBS,
                 max_region=RC.MAX_REGION, max_nodes=RACE_NODES, max_pairs=MAX_PAIRS, pad=2)
    _whole(got["n_pairs"], _listed(n_pairs, index, R, FILL32), ("race", S, asked, "n_pairs"))
    _whole(got["rows"], _listed(rows, index, R, FILL32), ("race", S, asked, "rows"))
    _whole(got["regions"], _listed(regions, index, R, FILL32), ("race", S, asked, "regions"))


# ---- secure --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _secure_tables(S):
    """(records [R], table int16 [R + 1, N, 4], sets uint32 [R + 1, 4, NW], counts int32 [R + 1, 8]); row R, out of range: zeros"""
    names, recs = SEC.case_records(S)
    R = W.secure_listed(len(recs), W.secure_geometry(S)[3])
    want = SEC.case_model(S, 0)
    out = []
    for k in ("table", "sets", "counts"):
        t = np.zeros((R + 1,) + want[k].shape[1:], want[k].dtype)
        t[:R] = want[k][:R]
        out.append(t)
    return (recs[:R],) + tuple(out)


@pytest.mark.parametrize("S", SIZES)
def test_secure_past_the_grid_cap(S):
    """k_secure with one workgroup per pair of candidates (sgo_secure_mode forces ch = pairs: 13 and 181), n * ch units behind the
    cap of 1 << 24: 1 296 001 rows at 5x5 -- unit 2^24 - 1 is pair 0 of row 1 290 555, whose other pairs belong to the second trip,
    and 5 445 rows lie wholly in it -- and 97 999 rows at 19x19 (row 92 691 astride the cap at pair 145, 5 307 rows behind it).
    Tables (259 MB and 283 MB), sets and counts whole against the model's rows of the case set, the two rows behind n included.
    These are the row counts first chosen, nothing was lowered: the launches take 12 ms and 55 ms, and what the 19x19 case spends
    beyond a second is the model's case set, which the process computes once."""
    from sejonggo_amd import _lib as L
    from tests import test_gpu_secure as G
    lib = L.require_gpu()
    ch, n, astride, first_whole, k0 = W.secure_geometry(S)
    recs, table, sets, counts = _secure_tables(S)
    R = len(recs)
    assert astride * ch < W.SECURE_CAP < first_whole * ch and n - first_whole >= 5000 and ch == (S * S + 1) // 2
    index = W.wrapped_index(n, first_whole, R)
    rec = W.record_of(index, R)
    # the expected rows themselves tell a row of the second trip from both rows its units have their twins in
    i = np.arange(astride, n)
    for back in (first_whole - 1, first_whole):
        a, b = rec[i], rec[np.maximum(i - back, 0)]
        assert ((table[a] != table[b]).any(axis=(1, 2)).mean() > 0.8), (S, back)
    prev = lib.sgo_secure_mode(-1)
    try:
        lib.sgo_secure_mode(ch)
        assert lib.sgo_secure_mode(-1) == ch
        got = G._run(S, recs, index, 0, pad=2)
    finally:
        lib.sgo_secure_mode(prev)
    _whole(got["counts"], _listed(counts, index, R, FILL32), ("secure", S, "counts"))
    _whole(got["sets"], _listed(sets, index, R, FILL32), ("secure", S, "sets"))
    _whole(got["table"], _listed(table, index, R, G.FILL16), ("secure", S, "table"))


# ---- rollout start ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(W.START_CASES))
def test_rollout_start_walk(case):
    """(a) 688 000 record words inside one trip but 1 075 000 ownership cells: `top` comes from own_n; (b) 2.1 M words, three trips;
    (c) 19x19, 1.15 M words and 1.08 M cells.  After each of two starts: the records are the listed sources, the list is the
    identity; after one step the result is per_src times the area score of each source -- the second as the first, not twice it"""
    import torch
    from sejonggo_amd import _lib as L
    from tests.test_gpu_rollout_step import _view
    L.require_gpu()
    lib = L.load()
    S, n_src, per_src, cap_src = W.START_CASES[case]
    N, RW = S * S, 16 * ((S * S + 31) // 32)
    src, owner = W.start_sources(S)
    index = W.wrapped_index(n_src, cap_src, len(src), with_out_of_range=False)
    n = n_src * per_src
    black = (owner[index] == 1).astype(np.int32)
    want_black, want_white = np.repeat((black * per_src)[:, None], N, 1), np.repeat(((1 - black) * per_src)[:, None], N, 1)
    sign = 2 * black.astype(np.int64) - 1
    want_sums = np.stack([black * per_src, (1 - black) * per_src, 0 * sign, sign * N * per_src, 0 * sign + N * N * per_src, 0 * sign + per_src,
                          0 * sign + per_src, 0 * sign + per_src], 1).astype(np.int64)
    want_rec = src[np.repeat(index, per_src)]
    h = C.c_void_p(lib.sgo_rollout_create(S, n, n_src, 0))
    assert h, lib.sgo_last_error().decode()
    try:
        table = torch.from_numpy(src.view(np.int32)).cuda()
        d_index = torch.from_numpy(index).cuda()
        policy = torch.zeros((n, N + 1), dtype=torch.float32, device="cuda")
        policy[:, N] = 1.0
        st = L.RolloutStatus()
        for seed in (1, 2):
            L.check(lib.sgo_rollout_start_dev(h, n_src, L.ptr(table), L.ptr(d_index), per_src, seed, 1, L.stream_ptr()), "sgo_rollout_start_dev")
            rec_p, idx_p = C.c_void_p(), C.c_void_p()
            assert lib.sgo_rollout_list(h, C.byref(rec_p), C.byref(idx_p)) == n
            torch.cuda.synchronize()
            _whole(_view(torch, rec_p.value, (n, RW)).cpu().numpy().view(np.uint32), want_rec, (case, seed, "records"))
            _whole(_view(torch, idx_p.value, (n,)).cpu().numpy(), np.arange(n, dtype=np.int32), (case, seed, "list"))
            L.check(lib.sgo_rollout_step(h, L.ptr(policy), 0, L.stream_ptr(), C.byref(st)), "sgo_rollout_step")
            assert (st.n_live, st.n_done, st.steps, st.error) == (0, n, 1, 0)
            got_black, got_white = np.full((n_src, N), -5, np.int32), np.full((n_src, N), -5, np.int32)
            sums = np.full((n_src, 8), -5, np.int64)
            L.check(lib.sgo_rollout_result(h, n_src, L.ptr(got_black), L.ptr(got_white), L.ptr(sums)), "sgo_rollout_result")
            _whole(got_black, want_black, (case, seed, "black_own"))
            _whole(got_white, want_white, (case, seed, "white_own"))
            _whole(sums, want_sums, (case, seed, "sums"))
    finally:
        lib.sgo_rollout_destroy(h)


# ---- RecordSet end to end -----------------------------------------------------------------------------------------------------
def test_record_set_past_the_caps():
    """the five golden 19x19 games repeated 80 times -- 400 games, 131 760 positions, one chunk: RecordSet.keys (131 360 rows, five
    trips of k_keys) and RecordSet.tactics(max_chains=16) (three trips of k_tactics_read).  Repetition 0 against the models on every
    fourth record, every later repetition bit-equal to repetition 0; 1 647 and 1 642 divide none of the trip lengths"""
    from sejonggo_amd.records import Record, RecordSet
    from tests.helpers import load
    S, REPS = 19, 80
    z = load("sgf_S19.npz")
    games, base = [], [0]
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        entries = [(S * S if y >= S else int(y) * S + int(x), int(c)) for x, y, c in mv]
        games.append(Record("g%d" % gi, S, entries, [False] * len(entries), list(range(1, len(entries) + 1)), None))
        base.append(base[-1] + len(entries) + 1)
    E, P = base[-1] - 5, base[-1]                                    # entries and records (positions) of one repetition
    assert (E, P) == (1642, 1647) and REPS * P == 131760 < 1 << 18
    assert 65535 % P == 1302 and 32768 % P == 1475 and 32768 % E != 0 and 65535 % E != 0
    gold_recs, gold = TC.golden_records(), TC.golden_model()
    rs = RecordSet(games * REPS, size=S)
    try:
        chunks = list(rs.keys())
        assert len(chunks) == 1 and not rs.refused
        ch = chunks[0]
        assert len(ch.key0) == REPS * E and ch.valid.all()
        # repetition 0: entry e of game g stands before record base[g] + e; every fourth record is a golden one
        rec0 = np.concatenate([base[g] + np.arange(len(games[g].entries)) for g in range(5)])
        assert np.array_equal(ch.index[:E], rec0)
        pick = np.flatnonzero(rec0 % 4 == 0)
        want = K.keys(S, gold_recs, rec0[pick] // 4, ch.action[:E][pick])
        for k, a in (("key0", ch.key0), ("canon", ch.canon), ("mask", ch.mask), ("canon_action", ch.canon_action)):
            _whole(np.asarray(a[:E][pick], dtype=want[k].dtype), want[k], ("record set keys", k))
            rep = np.asarray(a).reshape(REPS, E)
            assert (rep == rep[0]).all(), ("record set keys", k, np.flatnonzero((rep != rep[0]).any(axis=1))[:8])
        assert (ch.mask != 0).all() and len(np.unique(ch.canon[:E])) > E // 2
        chunks = list(rs.tactics(max_chains=16))
        assert len(chunks) == 1
        tt = chunks[0].tactics
        assert len(tt.n_chains) == REPS * P
        for j in range(len(gold["n_chains"])):
            k = min(16, len(gold["rows"][j]))
            assert tt.n_chains[4 * j] == gold["n_chains"][j] and np.array_equal(tt.libs[4 * j], gold["libs"][j]), j
            assert np.array_equal(tt.chains[4 * j, :k], gold["rows"][j][:k]), j
        for name, a in (("n_chains", tt.n_chains), ("libs", tt.libs), ("chains", tt.chains)):
            rep = np.asarray(a).reshape(REPS, -1)
            assert (rep == rep[0]).all(), ("record set tactics", name, np.flatnonzero((rep != rep[0]).any(axis=1))[:8])
        assert tt.n_chains[:P].max() > 4 and len(np.unique(tt.libs[:P], axis=0)) > P // 2
    finally:
        rs.close()
