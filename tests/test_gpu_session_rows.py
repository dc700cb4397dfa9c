"""GPU: the one row helper behind the six session analyses (csrc/sgo_session.hip session_rows) at the shapes where a slip in its
layout shows.  A 5x5 context: N = 25 is odd and NW = 1, so the byte column (libs), the int16 columns (values, the move table) and
the one-word bitsets all end off an 8-byte boundary.  Every sgo_session_X is called with a list of one slot and with a list of
three -- one slot twice and one that is no holding session -- into arrays filled with a sentinel: every SGO_OK row is the row
the matching sgo_X_dev gives for that slot's root record (the record sgo_records_replay writes after the same moves), the
refused row is SGO_ERR_STATE and holds the sentinel in every column, chain rows included.

The calls are ordered so that the session buffer grows between them: small ones first, then the move table for three slots and
the full chain table (at 5x5 the latter is what passes the buffer's first 4 KB), then the small ones again."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, N, NW = 5, 25, 1
SGO_ERR_STATE = -203
# slots 0..2 are set to these positions (y * S + x, colours alternate from black), slot 3 is never opened
MOVES = ([12, 7, 11], [6, 8, 16, 18, 12, 13, 7], [0, 1, 5, 6, 24, 2, 10, 11])
LISTS = ([0], [2, 3, 2], [1])
SENTINEL = {np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.uint32): 0xA5A5A5A5, np.dtype(np.uint64): 0xA5A5A5A5A5A5A5A5,
            np.dtype(np.int16): 0x5A5A, np.dtype(np.uint8): 0xA5}


def _filled(shape, dtype):
    return np.full(shape, SENTINEL[np.dtype(dtype)], dtype)


@pytest.fixture(scope="module")
def ctx():
    """(engine, backend, root): the sessions set up, the same move lists replayed as three records games, root[slot] the index of
    the record that holds the slot's position"""
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.records import DeviceRecords
    from sejonggo_amd.stub_nets import make_stub
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=4, sims=8, energy=4, symmetry="identity")
    be = DeviceRecords(S, len(MOVES), sum(len(m) for m in MOVES))
    try:
        n_entries = [len(m) for m in MOVES]
        off = np.concatenate([[0], np.cumsum(n_entries)[:-1]])
        colours = [1 if j % 2 == 0 else -1 for m in MOVES for j in range(len(m))]
        status, _ = be.replay(n_entries, off, [a for m in MOVES for a in m], colours)
        assert not status.any()
        root = [int(off[g]) + g + n_entries[g] for g in range(len(MOVES))]
        eng.open([0, 1, 2])
        st, _ = eng.setup([0, 1, 2], [list(m) for m in MOVES])
        assert not st.any()
        yield eng, be, root
    finally:
        eng.close()
        be.close()


def _check(slots, status, got, want):
    """got: {name: caller array}, want: {name: (rows of the _dev entry for the OK slots in list order, stored)}; stored[j] is how
    many leading items of OK row j the call writes (None: the whole row)"""
    ok = [i for i, s in enumerate(slots) if s != 3]
    assert status.tolist() == [0 if s != 3 else SGO_ERR_STATE for s in slots]
    for name, (rows, stored) in want.items():
        a = got[name]
        for j, i in enumerate(ok):
            if stored is None:
                assert np.array_equal(a[i], rows[j]), (name, slots, i)
            else:
                assert np.array_equal(a[i][:stored[j]], rows[j][:stored[j]]), (name, slots, i)
                assert (a[i][stored[j]:] == SENTINEL[a.dtype]).all(), (name, "behind the stored part", slots, i)
        for i in set(range(len(slots))) - set(ok):
            assert (a[i] == SENTINEL[a.dtype]).all(), (name, "refused row", slots, i)


def _host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _keys(L, lib, eng, be, root, slots):
    n, idx = len(slots), np.array([root[s] for s in slots if s != 3], np.int32)
    st, k0, cn, mk = _filled(n, np.int32), _filled(n, np.uint64), _filled(n, np.uint64), _filled(n, np.int32)
    assert lib.sgo_session_keys(eng.ctx, n, L.ptr(np.array(slots, np.int32)), L.ptr(st), L.ptr(k0), L.ptr(cn), L.ptr(mk), L.stream_ptr()) == 0
    key0, canon, mask, _ = be.keys(idx)
    _check(slots, st, {"key0": k0, "canon": cn, "mask": mk},
           {"key0": (_host(key0, np.uint64), None), "canon": (_host(canon, np.uint64), None), "mask": (_host(mask), None)})


def _tactics(L, lib, eng, be, root, slots, mc):
    n, idx = len(slots), np.array([root[s] for s in slots if s != 3], np.int32)
    st, libs, nch, chains = _filled(n, np.int32), _filled((n, N), np.uint8), _filled(n, np.int32), _filled((n, mc, 8), np.int32)
    assert lib.sgo_session_tactics(eng.ctx, n, L.ptr(np.array(slots, np.int32)), mc, L.ptr(st), L.ptr(libs), L.ptr(nch), L.ptr(chains),
                                   L.stream_ptr()) == 0
    w_libs, w_n, w_chains = (_host(t) for t in be.tactics(idx, mc))
    assert 2 not in slots or w_n.max() == 2                       # two chains in atari or with two liberties in slot 2's position
    _check(slots, st, {"libs": libs, "n_chains": nch, "chains": chains},
           {"libs": (w_libs, None), "n_chains": (w_n, None), "chains": (w_chains, [min(int(k), mc) for k in w_n])})


def _life(L, lib, eng, be, root, slots):
    n, idx = len(slots), np.array([root[s] for s in slots if s != 3], np.int32)
    st, sets, counts = _filled(n, np.int32), _filled((n, 4, NW), np.uint32), _filled((n, 8), np.int32)
    assert lib.sgo_session_life(eng.ctx, n, L.ptr(np.array(slots, np.int32)), L.ptr(st), L.ptr(sets), L.ptr(counts), L.stream_ptr()) == 0
    w_sets, w_counts = be.life(idx)
    _check(slots, st, {"sets": sets, "counts": counts}, {"sets": (_host(w_sets, np.uint32), None), "counts": (_host(w_counts), None)})


def _shapes(L, lib, eng, be, root, slots):
    from sejonggo_amd.shapes import Shape
    shape = Shape.parse("XO")
    n, idx = len(slots), np.array([root[s] for s in slots if s != 3], np.int32)
    st, hits, cover = _filled(n, np.int32), _filled((n, 4), np.int32), _filled((n, NW), np.uint32)
    s = shape.to_struct()
    assert lib.sgo_session_shapes(eng.ctx, n, L.ptr(np.array(slots, np.int32)), C.byref(s), L.ptr(st), L.ptr(hits), L.ptr(cover),
                                  L.stream_ptr()) == 0
    w_hits, w_cover = be.shapes(idx, shape)
    assert (_host(w_hits)[:, 0] > 0).any()
    _check(slots, st, {"hits": hits, "cover": cover}, {"hits": (_host(w_hits), None), "cover": (_host(w_cover, np.uint32), None)})


def _moves(L, lib, eng, be, root, slots, side):
    n, idx = len(slots), np.array([root[s] for s in slots if s != 3], np.int32)
    st, rows, counts = _filled(n, np.int32), _filled((n, N, 8), np.int16), _filled((n, 8), np.int32)
    assert lib.sgo_session_moves(eng.ctx, n, L.ptr(np.array(slots, np.int32)), side, L.ptr(st), L.ptr(rows), L.ptr(counts), L.stream_ptr()) == 0
    w_rows, w_counts = be.moves(idx, side)
    _check(slots, st, {"rows": rows, "counts": counts}, {"rows": (_host(w_rows), None), "counts": (_host(w_counts), None)})


def _influence(L, lib, eng, be, root, slots, lift):
    """lift: the dead sets go up as the call's input block -- per row the first stone of the slot's own move list"""
    n, idx = len(slots), np.array([root[s] for s in slots if s != 3], np.int32)
    dead = np.array([[1 << MOVES[s][0]] if s != 3 else [0] for s in slots], np.uint32) if lift else None
    st, values, sets, counts = _filled(n, np.int32), _filled((n, N), np.int16), _filled((n, 4, NW), np.uint32), _filled((n, 8), np.int32)
    assert lib.sgo_session_influence(eng.ctx, n, L.ptr(np.array(slots, np.int32)), L.ptr(dead), 5, 10, 21, L.ptr(st), L.ptr(values),
                                     L.ptr(sets), L.ptr(counts), L.stream_ptr()) == 0
    w_values, w_sets, w_counts = be.influence(idx, dead[[i for i, s in enumerate(slots) if s != 3]] if lift else None)
    _check(slots, st, {"values": values, "sets": sets, "counts": counts},
           {"values": (_host(w_values), None), "sets": (_host(w_sets, np.uint32), None), "counts": (_host(w_counts), None)})


def test_every_session_analysis_row_is_the_dev_entry_row_and_refused_rows_stay(ctx):
    from sejonggo_amd import _lib as L
    eng, be, root = ctx
    lib = L.require_gpu()

    def small(slots):
        _keys(L, lib, eng, be, root, slots)
        _life(L, lib, eng, be, root, slots)
        _shapes(L, lib, eng, be, root, slots)
        _tactics(L, lib, eng, be, root, slots, 1)                    # fewer chain rows than chains: min(n_chains, max_chains) rows
        _influence(L, lib, eng, be, root, slots, lift=len(slots) > 1)
        _moves(L, lib, eng, be, root, slots, 0)

    small(LISTS[0])
    _moves(L, lib, eng, be, root, LISTS[1], 1)                       # the largest 16-byte column ...
    _tactics(L, lib, eng, be, root, LISTS[1], L.TACTICS_MAX_CHAINS)  # ... and the table that outgrows the buffer's first 4 KB
    small(LISTS[2])
    small(LISTS[1])
    small(LISTS[0])
