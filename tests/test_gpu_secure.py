"""GPU: the securing-move kernels (include/sgo.h "securing moves", csrc/sgo_secure.hip) against the model (tests/secure_model.py)
word for word -- table, sets and counts -- at every board size and for both sides, on the case set tests/test_secure_model_power.py
shows to notice the model's fault switches (tests/secure_cases.py)."""
import numpy as np
import pytest

from tests import secure_cases as SC
from tests import secure_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG = -1
FILL16, FILL32 = 0x5A5A, 0x3C3C3C3C
KEYS = ("table", "sets", "counts")


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _filled(S, n, dev=None):
    """sentinel-filled outputs for n rows: numpy without a device, torch tensors on it"""
    NW = (S * S + 31) // 32
    if dev is None:
        return np.full((n, S * S, 4), FILL16, np.int16), np.full((n, 4, NW), FILL32, np.uint32), np.full((n, 8), FILL32, np.int32)
    import torch
    return (torch.full((n, S * S, 4), FILL16, dtype=torch.int16, device=dev), torch.full((n, 4, NW), FILL32, dtype=torch.int32, device=dev),
            torch.full((n, 8), FILL32, dtype=torch.int32, device=dev))


def _numpy(table, sets, counts):
    return {"table": table.cpu().numpy(), "sets": sets.cpu().numpy().view(np.uint32), "counts": counts.cpu().numpy()}


def _run(S, records, index, side, n=None, n_records=None, pad=2):
    """sgo_secure_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    n = (len(index) if index is not None else len(records)) if n is None else n
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev) if index is not None else None
    table, sets, counts = _filled(S, n + pad, dev)
    rc = lib.sgo_secure_dev(S, n, L.ptr(d_rec), len(records) if n_records is None else n_records, L.ptr(d_idx), side, L.ptr(table),
                            L.ptr(sets), L.ptr(counts), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return _numpy(table, sets, counts)


def _same(got, want, n, what):
    """every word of table, sets and counts; the rows behind n are as they were filled"""
    bad = np.flatnonzero((got["table"][:n] != want["table"][:n]).any(axis=(1, 2)))
    if len(bad):
        i = int(bad[0])
        a = int(np.flatnonzero((got["table"][i] != want["table"][i]).any(axis=1))[0])
        raise AssertionError((what, "table", bad[:8].tolist(), "row", i, "point", a, got["table"][i, a].tolist(), want["table"][i, a].tolist()))
    bad = np.flatnonzero((got["counts"][:n] != want["counts"][:n]).any(axis=1))
    assert len(bad) == 0, (what, "counts", bad[:8].tolist(), got["counts"][bad[0]].tolist(), want["counts"][bad[0]].tolist())
    bad = np.flatnonzero((got["sets"][:n] != want["sets"][:n]).any(axis=(1, 2)))
    assert len(bad) == 0, (what, "sets", bad[:8].tolist(), got["sets"][bad[0]].tolist(), want["sets"][bad[0]].tolist())
    assert (got["table"][n:] == FILL16).all() and (got["sets"][n:] == FILL32).all() and (got["counts"][n:] == FILL32).all(), (what, "rows behind n")


def _indexed(want, index, R):
    """the model's outputs of records 0 .. R - 1 re-listed through an index (out of range: the zero row)"""
    out = {k: np.zeros((len(index),) + want[k].shape[1:], want[k].dtype) for k in KEYS}
    for i, r in enumerate(index):
        if 0 <= r < R:
            for k in KEYS:
                out[k][i] = want[k][r]
    return out


@pytest.mark.parametrize("S", M.SIZES)
def test_case_set_word_for_word(S):
    """every constructed position in its four variants and the rule shapes, for side 0 and side 1: in order without an index list,
    then through a list that permutes them, repeats some and holds entries out of range; the host twin"""
    L, lib = _lib()
    names, recs = SC.case_records(S)
    R = len(recs)
    rng = np.random.RandomState(S)
    index = np.concatenate([rng.permutation(R), [-1, R, 0, 0, 2 ** 31 - 1, -2 ** 31, R - 1, 1, R + 7]]).astype(np.int64)
    for side in (0, 1):
        want = SC.case_model(S, side)
        _same(_run(S, recs, None, side), want, R, ("in order", side))
        _same(_run(S, recs, index.astype(np.int32), side), _indexed(want, index, R), len(index), ("indexed", side))
        table, sets, counts = _filled(S, R)
        assert lib.sgo_secure(S, R, L.ptr(np.ascontiguousarray(recs)), side, L.ptr(table), L.ptr(sets), L.ptr(counts)) == 0
        _same({"table": table, "sets": sets, "counts": counts}, want, R, ("host twin", side))


def test_golden_positions():
    """every 16th record of tactics_cases.golden_records(), 26 positions of the five golden 19x19 games; one call per side"""
    recs = SC.golden_sample()
    assert len(recs) == 26
    for side in (0, 1):
        _same(_run(19, recs, None, side), SC.golden_model(side), len(recs), ("golden", side))


def test_every_dealing_writes_the_same_words():
    """sgo_secure_mode: one workgroup per row (the longest pair loop), three (a stride that does not divide the pairs), one pair
    per workgroup, and the dealing by point index that idles on stones -- the words do not depend on the launch shape; a lone row
    and a row list with an out-of-range row in the middle"""
    L, lib = _lib()
    S = 9
    names, recs = SC.case_records(S)
    want = SC.case_model(S, 0)
    pick = np.array([names.index("capture_opens_eye_sb"), -1, names.index("cascade_sb"), names.index("empty_sb")], np.int32)
    prev = lib.sgo_secure_mode(-1)
    try:
        for mode in (1, 3, 41, 1000, 1 << 16 | 1, 1 << 16 | 5, 1 << 16, 0):
            lib.sgo_secure_mode(mode)
            assert lib.sgo_secure_mode(-1) == mode and lib.sgo_secure_mode(1 << 20) == mode and lib.sgo_secure_mode(2000) == mode
            _same(_run(S, recs, pick, 0), _indexed(want, pick, len(recs)), len(pick), ("mode", mode))
            _same(_run(S, recs, pick[:1], 0), _indexed(want, pick[:1], len(recs)), 1, ("mode, one row", mode))
    finally:
        lib.sgo_secure_mode(prev)


def test_row_counts_and_bad_arguments():
    """n of 0, 1, 2, 3, 7; n_records bounds the index; the refusals leave the outputs as they were"""
    import torch
    L, lib = _lib()
    S = 9
    names, recs = SC.case_records(S)
    want = SC.case_model(S, 0)
    idx = (np.arange(7) * 5 % len(recs)).astype(np.int32)
    for n in (0, 1, 2, 3, 7):
        _same(_run(S, recs, idx[:max(n, 1)], 0, n=n), _indexed(want, idx[:n], len(recs)), n, n)
    k = names.index("connect_sb")
    _same(_run(S, recs, np.array([k, k + 1], np.int32), 0, n_records=k + 1), _indexed(want, [k, -1], len(recs)), 2, "n_records")
    dev = torch.device("cuda", 0)
    d = torch.zeros(1024, dtype=torch.int32, device=dev)
    table, sets, counts = _filled(S, 2, dev)
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), kw.get("R", 1), None, kw.get("side", 0),   # noqa: E731
                         kw.get("table", P(table)), kw.get("sets", P(sets)), kw.get("counts", P(counts)), L.stream_ptr()]
    for bad in (dict(S=8), dict(S=0), dict(n=-1), dict(R=-1), dict(side=2), dict(side=-1), dict(rec=None), dict(table=None), dict(sets=None),
                dict(counts=None), dict(table=table.data_ptr() + 2), dict(table=table.data_ptr() + 4)):
        assert lib.sgo_secure_dev(*args(**bad)) == SGO_ERR_ARG, bad
    torch.cuda.synchronize()
    assert (table == FILL16).all() and (sets == FILL32).all() and (counts == FILL32).all()
    assert lib.sgo_secure_dev(*args()) == 0
    torch.cuda.synchronize()
    # the empty board: a lone stone proves nothing
    assert (table[0, :, 0] == M.ALLOWED).all() and not table[0, :, 1:].any() and (table[1] == FILL16).all()
    assert counts[0].tolist() == [0, 0, 0, S * S, 0, 0, 0, 0] and not sets[0].any() and (counts[1] == FILL32).all()
    h = np.zeros(1024, np.uint32)
    ht, hs, hc = _filled(S, 1)
    assert lib.sgo_secure(8, 1, P(h), 0, P(ht), P(hs), P(hc)) == SGO_ERR_ARG and lib.sgo_secure(S, -1, P(h), 0, P(ht), P(hs), P(hc)) == SGO_ERR_ARG
    assert lib.sgo_secure(S, 1, P(h), 2, P(ht), P(hs), P(hc)) == SGO_ERR_ARG and lib.sgo_secure(S, 1, None, 0, P(ht), P(hs), P(hc)) == SGO_ERR_ARG
    assert lib.sgo_secure(S, 1, P(h), 0, None, P(hs), P(hc)) == SGO_ERR_ARG and lib.sgo_secure(S, 1, P(h), 0, P(ht), None, P(hc)) == SGO_ERR_ARG
    assert lib.sgo_secure(S, 1, P(h), 0, P(ht), P(hs), None) == SGO_ERR_ARG
    assert lib.sgo_secure(S, 0, P(h), 0, P(ht), P(hs), P(hc)) == 0
    assert (ht == FILL16).all() and (hs == FILL32).all() and (hc == FILL32).all()


def test_capturable_in_a_graph():
    """the call alone in a captured graph (its two launches in order), replayed twice over re-filled outputs: the eager result"""
    import torch
    L, lib = _lib()
    S = 13
    names, recs = SC.case_records(S)
    want = SC.case_model(S, 0)
    R = len(recs)
    dev = torch.device("cuda", 0)
    eager = _run(S, recs, None, 0, pad=1)                            # first, so that the capture is not the kernels' first launch
    d_rec = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32)).to(dev)
    table, sets, counts = _filled(S, R + 1, dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.sgo_secure_dev(S, R, L.ptr(d_rec), R, None, 0, L.ptr(table), L.ptr(sets), L.ptr(counts), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    for _ in range(2):
        for t, fill in ((table, FILL16), (sets, FILL32), (counts, FILL32)):
            t.fill_(fill)
        g.replay()
        torch.cuda.synchronize()
        _same(_numpy(table, sets, counts), want, R, "graph replay")
    assert all(np.array_equal(eager[k], _numpy(table, sets, counts)[k]) for k in KEYS)


def test_python_surface():
    """secure.secure on host records through an index list, and the Secure readers on the named cases"""
    from sejonggo_amd.secure import secure
    S = 9
    names, recs = SC.case_records(S)
    k, c = names.index("connect_sb"), names.index("capture_opens_eye_sb")
    for side in (0, 1):
        want = SC.case_model(S, side)
        v = secure(S, recs, index=[k, -1, c], side=side)
        assert len(v) == 3 and not v.table[1].any() and not v.counts[1].any() and not v.sets[1].any()
        for i, r in ((0, k), (2, c)):
            assert all(np.array_equal(getattr(v, key)[i], want[key][r]) for key in KEYS)
    v = secure(S, recs, index=[k, c])
    assert v.best(0) == (11, 12) and v.gain(0, 2) == 11 and [a for a, _ in v.securing(0)] == [2, 11] and v.harmful(0) == []
    assert v.securing(0, 12) == [(11, 12)] and len(v.secured(0)) == 12
    assert v.harmful(1) == [(1, -int(v.counts[1, 0] + v.counts[1, 1]))] and v.count(1, "harmful") == 1
