"""GPU: what stands on the position keys -- records.RecordSet.book / duplicates on the device against the same set keyed by the
model (tests/keys_model.py), sgo_session_keys against sgo_keys on replayed records, and one `gtp --device` session that plays from
a book built from tests/golden/review_S19.sgf."""
import os

import numpy as np
import pytest

from tests import keys_model as K
from tests.helpers import GOLDEN, load
from tests.test_keys_host import BASE, eight_copies, line_of, record_of

pytestmark = pytest.mark.gpu

SGO_ERR_STATE = -203
RECORD = os.path.join(GOLDEN, "review_S19.sgf")


class ModelKeyed(object):
    """A replay backend whose records are the device's and whose keys are the model's: what RecordSet makes of it is the
    expectation for the all-device run."""

    def __init__(self, S, max_games, max_entries):
        from sejonggo_amd.records import DeviceRecords
        self.S, self.dev = S, DeviceRecords(S, max_games, max_entries)

    def replay(self, n_entries, off, actions, colors):
        out = self.dev.replay(n_entries, off, actions, colors)
        self.records = self.dev.records.cpu().numpy().view(np.uint32)[:int(np.sum(n_entries)) + len(n_entries)].copy()
        return out

    def keys(self, index, target=None):
        out = K.keys(self.S, self.records, index, target)
        return out["key0"], out["canon"], out["mask"], (out["canon_action"] if target is not None else None)

    def close(self):
        self.dev.close()


def _both(recs, S, **kw):
    from sejonggo_amd.records import RecordSet
    mg, me = kw.get("max_games", len(recs)), kw.get("max_entries", sum(len(r.entries) for r in recs))
    return RecordSet(recs, S, **kw), RecordSet(recs, S, backend=ModelKeyed(S, mg, max(me, max(len(r.entries) for r in recs))), **kw)


def _golden_records():
    z = load("sgf_S19.npz")
    S = int(z["size"])
    recs = []
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        entries = [(S * S if y >= S else int(y) * S + int(x), int(c)) for x, y, c in mv]
        recs.append(record_of("g%02d" % gi, entries, winner=(1, -1, None)[gi % 3], size=S))
    L = K.luts(S)
    recs.insert(3, record_of("g01_turned", [(int(L[6, a]), c) for a, c in recs[1].entries], winner=-1, size=S))
    return S, recs


def test_book_and_duplicates_on_the_device_equal_the_model_keyed_set():
    S = 7
    recs = eight_copies() + [record_of("changed", line_of(BASE[:-1] + [(6, 1)], 2)), record_of("short", line_of(BASE[:3], 3), winner=-1)]
    for kw in ({}, {"max_games": 1}, {"max_games": 3, "max_entries": 20}):
        dev, ref = _both(recs, S, **kw)
        try:
            book = dev.book()
            assert book == ref.book() and len(book) == len(BASE) + 1
            assert book.count.tolist().count(10) == 3 and book.count.tolist().count(9) == len(BASE) - 4
            assert dev.book(plies=3) == ref.book(plies=3) and dev.book(min_count=9) == ref.book(min_count=9)
            assert dev.duplicates() == ref.duplicates() == [["copy%d" % g for g in range(8)]]
            ch_d, ch_r = next(dev.keys()), next(ref.keys())
            for k in ("key0", "canon", "mask", "canon_action"):
                assert np.array_equal(getattr(ch_d, k), getattr(ch_r, k)), k
        finally:
            dev.close()
            ref.close()


def test_the_golden_records_as_a_book():
    S, recs = _golden_records()
    dev, ref = _both(recs, S)
    try:
        book, want = dev.book(), ref.book()
        assert book == want and int(book.count.sum()) == 6 * 29                  # nodes 1 .. 29 of six records
        assert book.count.max() >= 2                                             # the turned copy doubles a whole line
        assert dev.duplicates() == ref.duplicates() == [["g01", "g01_turned"]]
        split = _both(recs, S, max_games=2)
        try:
            assert split[0].book() == book and split[0].duplicates() == [["g01", "g01_turned"]]
        finally:
            split[0].close()
            split[1].close()
    finally:
        dev.close()
        ref.close()


def test_session_keys_equal_the_keys_of_the_replayed_records():
    """slots set up by sgo_session_setup from prefixes of one golden game against sgo_keys (the host twin) of the records
    sgo_records_replay wrote at the same plies, and against the model; a slot that is no session is refused and its row stays"""
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.records import DeviceRecords
    from sejonggo_amd.stub_nets import make_stub
    S, recs = _golden_records()
    game = recs[2]
    plies = [0, 1, 37, 120, len(game.entries)]
    acts, cols = [a for a, _ in game.entries], [c for _, c in game.entries]
    be = DeviceRecords(S, 1, len(acts))
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=7, sims=8, energy=4, symmetry="identity")
    try:
        status, _ = be.replay([len(acts)], [0], acts, cols)
        assert not status.any()
        rows = np.ascontiguousarray(be.records.cpu().numpy().view(np.uint32)[plies])
        lib = L.require_gpu()
        k0, cn, mk = np.zeros(5, np.uint64), np.zeros(5, np.uint64), np.zeros(5, np.int32)
        assert lib.sgo_keys(S, 5, L.ptr(rows), None, L.ptr(k0), L.ptr(cn), L.ptr(mk), None) == 0
        want = K.keys(S, rows)
        assert np.array_equal(k0, want["key0"]) and np.array_equal(cn, want["canon"]) and np.array_equal(mk, want["mask"])
        slots = [5, 0, 3, 1, 4]
        eng.open(slots)
        st, _ = eng.setup(slots, [acts[:p] for p in plies], [cols[:p] for p in plies])
        assert not st.any()
        got = eng.keys(slots)
        assert not got["status"].any()
        assert np.array_equal(got["key0"], k0) and np.array_equal(got["canon"], cn) and np.array_equal(got["mask"], mk)
        # slots 2 and 6 were never opened; a slot may be listed twice; refused rows are left as they were filled
        ask = np.array([2, 3, 6, 3, 5], np.int32)
        out = {"status": np.full(5, 77, np.int32), "key0": np.full(5, 11, np.uint64), "canon": np.full(5, 12, np.uint64),
               "mask": np.full(5, 13, np.int32)}
        rc = lib.sgo_session_keys(eng.ctx, 5, L.ptr(ask), L.ptr(out["status"]), L.ptr(out["key0"]), L.ptr(out["canon"]),
                                  L.ptr(out["mask"]), L.stream_ptr())
        assert rc == 0 and out["status"].tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        assert out["key0"].tolist() == [11, int(k0[2]), 11, int(k0[2]), int(k0[0])]
        assert out["canon"].tolist() == [12, int(cn[2]), 12, int(cn[2]), int(cn[0])]
        assert out["mask"].tolist() == [13, int(mk[2]), 13, int(mk[2]), 255]
        # a move changes the key, the tree's state does not
        assert not eng.play([3], [acts[37]], [cols[37]]).any()
        one = eng.keys([3])
        assert one["key0"][0] == K.keys(S, be.records.cpu().numpy().view(np.uint32)[38:39])["key0"][0]
        assert lib.sgo_session_keys(eng.ctx, 1, L.ptr(np.array([7], np.int32)), L.ptr(out["status"]), L.ptr(out["key0"]),
                                    L.ptr(out["canon"]), L.ptr(out["mask"]), L.stream_ptr()) == -1
    finally:
        eng.close()
        be.close()


def test_gtp_device_session_plays_from_the_book(tmp_path):
    """a book of the first four moves of the committed record: sgo-book lists them, genmove plays them without a search -- in the
    frame the first answer chose, since the empty board does not tell the eight orientations apart -- and searches afterwards"""
    from sejonggo_amd import gtp, records as R, symmetry
    from sejonggo_amd.conf import conf
    from sejonggo_amd.stub_nets import make_stub
    with open(RECORD) as f:
        rec = R.parse_record(f.read(), "review")
    S = rec.size
    rs = R.RecordSet([rec], S)
    try:
        book = rs.book(plies=5)
    finally:
        rs.close()
    assert len(book) == 4 and book.count.tolist() == [1] * 4
    path = str(tmp_path / "book.npz")
    book.save(path)
    keep, keep_sym = dict(conf), list(symmetry.SYMMETRIES)
    symmetry.SYMMETRIES[:] = symmetry.SYMMETRIES[0:1]
    conf.update({'SIZE': S, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", S), size=S, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev, book=path)
        L = K.luts(S)
        frames = list(range(8))
        z = {1: (1, 0), -1: (0, 1), None: (0, 0)}
        for j in range(4):
            a, colour = rec.entries[j]
            w, l = z[rec.winner if rec.winner is None else rec.winner * colour]
            listed = e.parse_command("sgo-book")
            reply = e.parse_command("genmove %s" % ("B" if colour == 1 else "W"))
            frames = [g for g in frames if reply == "= %s\n\n" % e._vertex(int(L[g, a]))]
            assert frames, (j, reply)
            assert listed == "= %s 1 %d %d\n\n" % (reply[2:].strip(), w, l)
            assert dev.moves[-1] == (int(L[frames[0], a]), colour)
        assert int(dev.engine.status.total_evals) == 0 and dev.move == 5
        assert e.parse_command("sgo-book") == "=\n\n"
        reply = e.parse_command("genmove B")
        assert reply.startswith("= ") and int(dev.engine.status.total_evals) > 0 and dev.move == 6
    finally:
        dev.close()
        symmetry.SYMMETRIES[:] = keep_sym
        conf.clear()
        conf.update(keep)
