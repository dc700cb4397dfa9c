"""GPU: the position-key kernel (include/sgo.h "position keys", csrc/sgo_keys.hip) against the model (tests/keys_model.py) bit for
bit at every board size: 5 (the flag and the stones share a word), 7 (rows straddle the word boundary), 9, 13 and 19 (twelve
words, nine live bits in the last).  The case set is the one tests/test_keys_model_power.py shows to notice every fault switch."""
import numpy as np
import pytest

from tests import keys_model as K
from tests import records_model as M
from tests.helpers import load

pytestmark = pytest.mark.gpu

SGO_ERR_ARG = -1
FILL64, FILL32 = 0x5A5A5A5A5A5A5A5A, 0x3C3C3C3C


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _run(S, records, index, target, n=None, n_records=None, pad=3):
    """sgo_keys_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    n = (len(index) if index is not None else len(records)) if n is None else n
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev) if index is not None else None
    d_tgt = torch.from_numpy(np.ascontiguousarray(target, np.int32)).to(dev) if target is not None else None
    key0 = torch.full((n + pad,), FILL64, dtype=torch.int64, device=dev)
    canon = torch.full((n + pad,), FILL64, dtype=torch.int64, device=dev)
    mask = torch.full((n + pad,), FILL32, dtype=torch.int32, device=dev)
    action = torch.full((n + pad,), FILL32, dtype=torch.int32, device=dev)
    rc = lib.sgo_keys_dev(S, n, L.ptr(d_rec), len(records) if n_records is None else n_records, L.ptr(d_idx), L.ptr(d_tgt),
                          L.ptr(key0), L.ptr(canon), L.ptr(mask), L.ptr(action) if target is not None else None, L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return {"key0": key0.cpu().numpy().view(np.uint64), "canon": canon.cpu().numpy().view(np.uint64), "mask": mask.cpu().numpy(),
            "canon_action": action.cpu().numpy()}


def _same(got, want, n, what, targets=True):
    for k in ("key0", "canon", "mask") + (("canon_action",) if targets else ()):
        bad = np.flatnonzero(got[k][:n] != want[k][:n])
        assert len(bad) == 0, (what, k, bad[:8], got[k][bad[:4]], want[k][bad[:4]])
    # rows beyond n are untouched (and canon_action everywhere when there are no targets)
    assert (got["key0"][n:] == FILL64).all() and (got["canon"][n:] == FILL64).all() and (got["mask"][n:] == FILL32).all()
    assert (got["canon_action"][n if targets else 0:] == FILL32).all()


@pytest.mark.parametrize("S", K.SIZES)
def test_case_set_bit_for_bit(S):
    """the empty board, one stone per symmetry class, positions invariant under each subgroup, fully symmetric positions and the
    reference's random positions, for both sides to move, over a random pattern in planes 2..15 and the padding bits; every
    target of -1 .. N + 1; an index list with repeats and entries out of range; both kernel forms; the host twin"""
    L, lib = _lib()
    names, recs = K.case_records(S)
    R = len(recs)
    index, target = K.case_rows(S, names, R)
    index = np.concatenate([index, [-1, R, R + 5, 0, 0, 2 ** 31 - 1, -2 ** 31, 1]]).astype(np.int32)
    target = np.concatenate([target, [0, 1, S * S, 3, S * S, 0, 0, -7]]).astype(np.int32)
    want = K.keys(S, recs, index, target)
    assert want["mask"][0] == 255 and (want["mask"][-8:] == [0, 0, 0, 255, 255, 0, 0, 255]).all()
    n = len(index)
    prev = lib.sgo_keys_mode(0)
    try:
        got = _run(S, recs, index, target)
        _same(got, want, n, "table")
        assert lib.sgo_keys_mode(1) == 0
        _same(_run(S, recs, index, target), want, n, "inline")
    finally:
        lib.sgo_keys_mode(prev)
    # the host twin: the records in order
    t2 = np.array([i % (S * S + 3) - 1 for i in range(R)], np.int32)
    k0, cn = np.zeros(R, np.uint64), np.zeros(R, np.uint64)
    mk, ca = np.zeros(R, np.int32), np.zeros(R, np.int32)
    assert lib.sgo_keys(S, R, L.ptr(np.ascontiguousarray(recs)), L.ptr(t2), L.ptr(k0), L.ptr(cn), L.ptr(mk), L.ptr(ca)) == 0
    dev = _run(S, recs, None, t2)
    w2 = K.keys(S, recs, None, t2)
    for k, a in (("key0", k0), ("canon", cn), ("mask", mk), ("canon_action", ca)):
        assert np.array_equal(a, dev[k][:R]) and np.array_equal(a, w2[k]), k


def test_row_counts_null_lists_and_bad_arguments():
    """n of 0, 1, 2, 3 and 65 (a lone half-wave; more than one workgroup of eight rows); no index list; no targets and no
    canon_action array; the refusals"""
    import torch
    L, lib = _lib()
    S = 9
    names, recs = K.case_records(S)
    idx = (np.arange(65) * 7 % len(recs)).astype(np.int32)
    tgt = (np.arange(65) * 5 % (S * S + 1)).astype(np.int32)
    want = K.keys(S, recs, idx, tgt)
    for n in (0, 1, 2, 3, 65):
        _same(_run(S, recs, idx[:max(n, 1)], tgt[:max(n, 1)], n=n), want, n, n)
        _same(_run(S, recs, idx[:max(n, 1)], None, n=n), want, n, (n, "no targets"), targets=False)
    plain = K.keys(S, recs, None, None)
    _same(_run(S, recs, None, None, n=65), plain, 65, "no lists", targets=False)
    # n_records bounds the index, not the array's length
    got = _run(S, recs, np.array([3, 4, 5], np.int32), None, n_records=5)
    assert got["mask"][:3].tolist() == [plain["mask"][3], plain["mask"][4], 0] and got["canon"][2] == 0 and got["key0"][2] == 0
    dev = torch.device("cuda", 0)
    d = torch.zeros(64, dtype=torch.int64, device=dev)
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), 1, None, kw.get("tgt", None), kw.get("k0", P(d)),   # noqa: E731
                         kw.get("cn", P(d)), kw.get("mk", P(d)), kw.get("ca", None), L.stream_ptr()]
    assert lib.sgo_keys_dev(*args()) == 0
    for bad in (dict(S=8), dict(n=-1), dict(rec=None), dict(k0=None), dict(cn=None), dict(mk=None), dict(tgt=P(d))):
        assert lib.sgo_keys_dev(*args(**bad)) == SGO_ERR_ARG, bad
    assert lib.sgo_keys_dev(*args(tgt=P(d), ca=P(d))) == 0
    h = np.zeros(64, np.uint64)
    assert lib.sgo_keys(8, 1, P(h), None, P(h), P(h), P(h), None) == SGO_ERR_ARG
    assert lib.sgo_keys(S, 1, P(h), P(h), P(h), P(h), P(h), None) == SGO_ERR_ARG
    assert lib.sgo_keys(S, 0, P(h), None, P(h), P(h), P(h), None) == 0
    torch.cuda.synchronize()


def test_the_golden_records_in_one_launch():
    """the five 19x19 records of the reference replayed by sgo_records_replay, every record (about 1 650) keyed in one launch
    through DeviceRecords.keys, the recorded move as the target; the model reads the records the replay wrote"""
    from sejonggo_amd.records import DeviceRecords
    z = load("sgf_S19.npz")
    S = int(z["size"])
    games = []
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        games.append(([S * S if y >= S else int(y) * S + int(x) for x, y, _ in mv], [int(c) for _, _, c in mv]))
    n, off, acts, cols = M.lists_of(games)
    total = int(n.sum())
    be = DeviceRecords(S, 5, total)
    try:
        status, _ = be.replay(n, off, acts, cols)
        assert not status.any()
        R = total + 5
        target = np.full(R, S * S, np.int32)                       # the final positions get the pass
        for g in range(5):
            target[int(off[g]) + g:int(off[g]) + g + int(n[g])] = games[g][0]
        key0, canon, mask, action = be.keys(np.arange(R, dtype=np.int32), target)
        recs = be.records.cpu().numpy().view(np.uint32)[:R]
        want = K.keys(S, recs, None, target)
        assert np.array_equal(key0.cpu().numpy().view(np.uint64), want["key0"])
        assert np.array_equal(canon.cpu().numpy().view(np.uint64), want["canon"])
        assert np.array_equal(mask.cpu().numpy(), want["mask"]) and np.array_equal(action.cpu().numpy(), want["canon_action"])
        assert want["mask"][0] == 255 and (want["mask"] != 0).all()
        assert len(np.unique(want["canon"])) > R // 2              # the games differ
        # no targets: canon_action is None, the rest unchanged; an empty list is no launch
        k0b, cb, mb, ab = be.keys(np.arange(R, dtype=np.int32))
        assert ab is None and np.array_equal(cb.cpu().numpy(), canon.cpu().numpy()) and np.array_equal(mb.cpu().numpy(), mask.cpu().numpy())
        assert [int(t.shape[0]) for t in be.keys(np.zeros(0, np.int32))[:3]] == [0, 0, 0]
    finally:
        be.close()
